"""The layouts of the data column calls, in plain Python: T from the blob-major layout of the cell calls (piece k of item i at
piece_bytes * (128 * i + k)) to the column-major one (the piece of column c, row b at piece_bytes * (c * n + b)), its inverse, and the
sidecar lists `Setup.verify_data_columns` takes.  Pieces are cells (2048 bytes) or proofs (48)."""
CELLS = 128
CELL = 2048
PROOF = 48


def to_columns(blob_major, n, piece):
    """T: n items of 128 pieces each -> 128 columns of n pieces each"""
    assert len(blob_major) == n * CELLS * piece
    return b"".join(blob_major[piece * (CELLS * b + c): piece * (CELLS * b + c + 1)] for c in range(CELLS) for b in range(n))


def to_rows(column_major, n, piece):
    """T^-1"""
    assert len(column_major) == n * CELLS * piece
    return b"".join(column_major[piece * (c * n + b): piece * (c * n + b + 1)] for b in range(n) for c in range(CELLS))


def column_at(n, row, at, piece=CELL):
    """the address map of the kernels: where byte `at` of an item's 128 * piece bytes lies in a column matrix of n rows"""
    return ((at // piece) * n + row) * piece + at % piece


def sidecars(cells_cm, proofs_cm, n, columns=range(CELLS)):
    """column matrices -> [(column_index, [n cells], [n proofs])]"""
    return [(c, [cells_cm[CELL * (c * n + b): CELL * (c * n + b + 1)] for b in range(n)],
             [proofs_cm[PROOF * (c * n + b): PROOF * (c * n + b + 1)] for b in range(n)]) for c in columns]


def from_sidecars(columns, n, fill=0):
    """the column matrices (cells, proofs) and the 16-byte mask of the given sidecars; absent columns are `fill` bytes"""
    cells, proofs, mask = bytearray([fill]) * (n * CELLS * CELL), bytearray([fill]) * (n * CELLS * PROOF), bytearray(16)
    for c, col_cells, col_proofs in columns:
        assert len(col_cells) == n and len(col_proofs) == n
        cells[CELL * c * n: CELL * (c + 1) * n] = b"".join(col_cells)
        proofs[PROOF * c * n: PROOF * (c + 1) * n] = b"".join(col_proofs)
        mask[c >> 3] |= 1 << (c & 7)
    return bytes(cells), bytes(proofs), bytes(mask)


def mask_of_columns(columns):
    mask = bytearray(16)
    for c in columns:
        mask[c >> 3] |= 1 << (c & 7)
    return bytes(mask)


def complement(mask):
    return bytes(b ^ 0xFF for b in mask)


def laid(full_cm, rest_cm, n, columns, piece=PROOF, zero_rows=()):
    """a column matrix after a call that writes `columns`: the bytes of `full_cm` there (zero bytes in `zero_rows`), `rest_cm` elsewhere"""
    out = bytearray(rest_cm)
    for c in columns:
        for b in range(n):
            at = piece * (c * n + b)
            out[at: at + piece] = bytes(piece) if b in zero_rows else full_cm[at: at + piece]
    return bytes(out)
