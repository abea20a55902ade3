"""Expected values of recover_cells (EIP-7594) for the recovery tests: a big-int restatement of the spec's `recover_polynomialcoeff`
(specs/fulu/polynomial-commitments-sampling.md) done the long way -- the vanishing polynomial over the missing cells, 8192-point
transforms, the coset shift 7 -- followed by the re-evaluation of `recover_cells_and_kzg_proofs`.  It shares nothing with the engine's
half-size route but the oracle's modulus and root-of-unity function.  Also: the masks the host program and the GPU tests use."""
import random

from oracle.pyref import domain
from oracle.pyref.bls import R

N = 4096
EXT = 8192
CELLS = 128
PER_CELL = 64
CELL = 2048
SHIFT = 7  # the spec's PRIMITIVE_ROOT_OF_UNITY as coset shift
NOT_ENOUGH = 8
INVALID_ELEMENT = 2
INCONSISTENT = 9


def _brp(values):
    return domain.bit_reversal_permutation(values)


def _fft(values, roots):
    """spec `_fft_field`: values = coefficients, roots = the len(values) powers of a primitive root -> evaluations, natural order"""
    if len(values) == 1:
        return list(values)
    left = _fft(values[::2], roots[::2])
    right = _fft(values[1::2], roots[::2])
    half = len(left)
    out = [0] * len(values)
    for i in range(half):
        y = right[i] * roots[i] % R
        out[i] = (left[i] + y) % R
        out[i + half] = (left[i] - y) % R
    return out


def fft(values, roots, inv=False):
    if not inv:
        return _fft(values, roots)
    ninv = pow(len(values), -1, R)
    return [v * ninv % R for v in _fft(values, [roots[0]] + list(roots[:0:-1]))]


def coset_fft(values, roots, inv=False):
    if not inv:
        f, shifted = 1, []
        for v in values:
            shifted.append(v * f % R)
            f = f * SHIFT % R
        return fft(shifted, roots)
    out = fft(values, roots, inv=True)
    hi, f = pow(SHIFT, -1, R), 1
    for i in range(len(out)):
        out[i] = out[i] * f % R
        f = f * hi % R
    return out


def vanishing_polynomialcoeff(xs):
    p = [1]
    for x in xs:
        p = [0] + p
        for i in range(len(p) - 1):
            p[i] = (p[i] - p[i + 1] * x) % R
    return p


def recover_polynomialcoeff(cell_indices, cosets_evals):
    """the spec's function: cell_indices (any order, distinct), cosets_evals[i] = the 64 elements of cell cell_indices[i]"""
    roots_ext = domain.roots_of_unity(EXT)
    rbo = [0] * EXT
    for c, evals in zip(cell_indices, cosets_evals):
        rbo[c * PER_CELL: (c + 1) * PER_CELL] = evals
    evaluation = _brp(rbo)
    missing = [domain.bit_reversal_permutation_index(c, CELLS) for c in range(CELLS) if c not in set(cell_indices)]
    roots_reduced = domain.roots_of_unity(CELLS)
    short = vanishing_polynomialcoeff([roots_reduced[i] for i in missing])
    zero_poly = [0] * EXT
    for i, coeff in enumerate(short):
        zero_poly[i * PER_CELL] = coeff
    zero_eval = fft(zero_poly, roots_ext)
    times_zero = [a * b % R for a, b in zip(zero_eval, evaluation)]
    times_zero_coeff = fft(times_zero, roots_ext, inv=True)
    times_zero_coset = coset_fft(times_zero_coeff, roots_ext)
    zero_coset = coset_fft(zero_poly, roots_ext)
    quotient = [a * pow(b, -1, R) % R for a, b in zip(times_zero_coset, zero_coset)]
    return coset_fft(quotient, roots_ext, inv=True)[:N]


def recover_cells_bytes(cells, mask):
    """cells: 262,144 bytes (absent cells may hold anything), mask: 16 bytes -> the 262,144 bytes of the recovered cell set.  For inputs
    the engine accepts."""
    indices = [c for c in range(CELLS) if present(mask, c)]
    evals = [[int.from_bytes(cells[CELL * c + 32 * i: CELL * c + 32 * i + 32], "big") for i in range(PER_CELL)] for c in indices]
    coeff = recover_polynomialcoeff(indices, evals)
    ext = _brp(fft(coeff + [0] * N, domain.roots_of_unity(EXT)))
    return b"".join(v.to_bytes(32, "big") for v in ext)


# ---- masks --------------------------------------------------------------------------------------------------------------------------
def mask_of(missing):
    m = bytearray(b"\xff" * 16)
    for c in missing:
        m[c >> 3] &= ~(1 << (c & 7)) & 0xFF
    return bytes(m)


def present(mask, c):
    return (mask[c >> 3] >> (c & 7)) & 1 == 1


def random_missing(seed, count=64):
    return sorted(random.Random(seed).sample(range(CELLS), count))


def host_masks():
    """name -> mask: the set the issue lists for the host program"""
    return {
        "none missing": mask_of([]),
        "0..63 missing": mask_of(range(64)),
        "64..127 missing": mask_of(range(64, 128)),
        "even missing": mask_of(range(0, 128, 2)),
        "127 missing": mask_of([127]),
        "random 64 missing": mask_of(random_missing(0x7594)),
    }


def knock_out(cells, mask, fill=0xFF):
    """the cell set with every absent cell overwritten by `fill` bytes"""
    out = bytearray(cells)
    for c in range(CELLS):
        if not present(mask, c):
            out[CELL * c: CELL * (c + 1)] = bytes([fill]) * CELL
    return bytes(out)
