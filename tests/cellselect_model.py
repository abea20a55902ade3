"""The `want` masks of the select forms of the cell-proof calls and a plain restatement of what the host derives from them
(kateth_amd/csrc/cellproof_plan.hpp): the pair list and the pass plan.  Shared by tests/test_cellproofs_select_host.py, which holds the
C++ header to this model, and tests/test_gpu_cellproofs_select.py, which uses the same masks on the device."""
import random

CELLS = 128
MAX_ITEMS = 128
SEED = 0x7594


def mask_of(cells):
    """16 bytes: cell c is bit c & 7, least significant first, of byte c >> 3"""
    m = bytearray(16)
    for c in cells:
        assert 0 <= c < CELLS
        m[c >> 3] |= 1 << (c & 7)
    return bytes(m)


def cells_of(mask):
    return [c for c in range(CELLS) if (mask[c >> 3] >> (c & 7)) & 1]


def random_cells(count, tag=0):
    return sorted(random.Random(SEED * 1000 + 131 * count + tag).sample(range(CELLS), count))


ALL, EMPTY = list(range(CELLS)), []
TWELVE = random_cells(12)
# per-item cell sets over five items: an empty mask between non-empty ones, first and last; bit 0, bit 127, two byte boundaries
ASSIGNMENTS = [
    [ALL, EMPTY, [0], [127], [7, 8]],
    [EMPTY, [63, 64], TWELVE, ALL, EMPTY],
    [[7, 8], EMPTY, [127], EMPTY, [0]],
]
# six items whose passes at KATETH_AMD_CELLPROOF_PASS=1 (128 vectors) are: 100 + 0 + 28 (an exact fill with an empty-mask item inside),
# 1, 128 (a full pass of one item), 127 (ragged)
PASS_COUNTS = [100, 0, 28, 1, 128, 127]
PASS_CELLS = [random_cells(k, tag=7) for k in PASS_COUNTS]
PASS_PLAN_AT_1 = [(3, 128), (1, 1), (1, 128), (1, 127)]


def masks_of(cell_sets):
    return b"".join(mask_of(c) for c in cell_sets)


def plan(masks, P):
    """[(items, vectors)]: consecutive items share a pass while its vectors stay <= 128 P and its items <= 128"""
    n = len(masks) // 16
    P = max(1, min(P, MAX_ITEMS))
    out, items, vectors = [], 0, 0
    for i in range(n):
        v = len(cells_of(masks[16 * i: 16 * i + 16]))
        if items and (vectors + v > CELLS * P or items == MAX_ITEMS):
            out.append((items, vectors))
            items, vectors = 0, 0
        items, vectors = items + 1, vectors + v
    if items:
        out.append((items, vectors))
    return out


def even_plan(n, P):
    return [(min(P, n - at), CELLS * min(P, n - at)) for at in range(0, n, P)]


def pairs(masks, passes):
    """the pair lists of all passes, one behind the other: 128 * (item within its pass) + cell, in item order, then cell order"""
    out, base = [], 0
    for items, _ in passes:
        for i in range(items):
            out += [CELLS * i + c for c in cells_of(masks[16 * (base + i): 16 * (base + i) + 16])]
        base += items
    return out
