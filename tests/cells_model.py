"""Expected values of compute_cells (EIP-7594) for the cells tests: a big-int transform written after the three steps of the issue --
decimation-in-time inverse transform with omega_4096^-1 on the blob as it lies in memory, the twist omega_8192^k / 4096, decimation-in-
frequency forward transform with omega_4096 -- with nothing shared with the engine but the oracle's modulus and root-of-unity function."""
import functools

from oracle.pyref import domain
from oracle.pyref.bls import R  # noqa: F401 (re-exported: cm.R)

BLOB = 131072
CELL = 2048
CELLS = 128
OMEGA_8192_HEX = "485d512737b1da3d2ccddea2972e89ed146b58bc434906ac6fdd00bfc78c8967"


def extension(values):
    """values = p at roots_of_unity_brp(n)  ->  p at omega_2n * roots_of_unity_brp(n), in the same order"""
    n = len(values)
    g = domain.primitive_root_of_unity(2 * n)
    w = g * g % R
    x = list(values)
    wi = pow(w, -1, R)
    m = 1
    while m < n:  # decimation in time: bit-reversed in, natural out
        wm = pow(wi, n // (2 * m), R)
        for k in range(0, n, 2 * m):
            t = 1
            for j in range(m):
                u, v = x[k + j], x[k + j + m] * t % R
                x[k + j], x[k + j + m] = (u + v) % R, (u - v) % R
                t = t * wm % R
        m *= 2
    ninv, t = pow(n, -1, R), 1
    for k in range(n):
        x[k] = x[k] * t % R * ninv % R
        t = t * g % R
    m = n // 2
    while m >= 1:  # decimation in frequency: natural in, bit-reversed out
        wm = pow(w, n // (2 * m), R)
        for k in range(0, n, 2 * m):
            t = 1
            for j in range(m):
                u, v = x[k + j], x[k + j + m]
                x[k + j], x[k + j + m] = (u + v) % R, (u - v) * t % R
                t = t * wm % R
        m //= 2
    return x


def elements(blob):
    return [int.from_bytes(blob[32 * i: 32 * i + 32], "big") for i in range(len(blob) // 32)]


def to_bytes(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


@functools.lru_cache(maxsize=None)
def extension_bytes(blob):
    """the 131,072 bytes of cells 64..127 of a valid blob"""
    return to_bytes(extension(elements(blob)))


def cells_bytes(blob):
    """all 262,144 bytes; a blob with an element >= r gives zeros"""
    if any(v >= R for v in elements(blob)):
        return bytes(2 * BLOB)
    return bytes(blob) + extension_bytes(bytes(blob))


@functools.lru_cache(maxsize=None)
def roots_brp():
    return tuple(domain.bit_reversal_permutation(domain.roots_of_unity(4096)))


def closed_form_blobs():
    """name -> (blob, extension half known in closed form or None)"""
    g = domain.primitive_root_of_unity(8192)
    rb = roots_brp()
    return {
        "zero": (bytes(BLOB), bytes(BLOB)),
        "r_minus_1": (to_bytes([R - 1] * 4096), to_bytes([R - 1] * 4096)),  # a constant polynomial
        "x": (to_bytes(rb), to_bytes([g * v % R for v in rb])),  # p = X
        "x4095": (to_bytes([pow(v, 4095, R) for v in rb]), to_bytes([pow(g * v % R, 4095, R) for v in rb])),  # p = X^4095
    }
