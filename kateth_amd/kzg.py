"""Host-side mirror of kateth's `kzg::Setup` over the C ABI (ctypes).

Method names, argument meaning and error behaviour follow the reference:

    Setup.load_json(path)                        src/kzg/setup.rs:46-82
    Setup.blob_to_commitment(blob)               src/kzg/setup.rs:167-171   (+ compress, src/bls.rs:491-503)
    Setup.blob_proof(blob, commitment48)         src/kzg/setup.rs:177-183
    Setup.blob_sidecar(blob)                     :167-171 then :177-183 on the same blob, + EIP-4844 kzg_to_versioned_hash
    Setup.compute_cells(blob)                    EIP-7594 compute_cells (specs/fulu/polynomial-commitments-sampling.md)
    Setup.recover_cells(cell_indices, cells)     EIP-7594 recover_cells_and_kzg_proofs, its cells half (same document)
    Setup.proof(blob, z32)                       src/kzg/setup.rs:185-194
    Setup.verify_proof(proof, commitment, z, y)  src/kzg/setup.rs:96-113
    Setup.verify_blob_proof(blob, c, p)          src/kzg/setup.rs:208-221
    Setup.verify_blob_proof_batch(blobs, cs, ps) src/kzg/setup.rs:247-275
    Setup.verify_proof_batch(ps, cs, zs, ys)     src/kzg/setup.rs:115-161 behind :96-113 per tuple
    Setup.verify_cell_proof_batch(cs, idx, cells, ps)  EIP-7594 verify_cell_kzg_proof_batch (same document as compute_cells)
    Setup.verify_cell_proof_batch_each(cs, idx, cells, ps)  the same, one verdict (or error) per tuple
    Setup.verify_cell_proof_batch_rows(cs, rows, idx, cells, ps)  the same check on a block's commitment LIST and an index per cell
    Setup.verify_cell_proof_batch_rows_each(cs, rows, idx, cells, ps)  that form with one verdict (or error) per cell
    Setup.verify_data_columns(cs, columns)  ... built from column sidecars (column index, cells, proofs)

Points cross this boundary in their 48-byte compressed form (what every caller
of the reference does next: benches/kzg.rs:25-32, src/kzg/setup.rs:341-343).
The `*_batch` / `*_dev` methods expose the batch-level C entry points directly;
the single-item methods are batches of one.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import List, Optional, Sequence, Tuple, Union

BYTES_PER_BLOB = 131072
CELLS_PER_EXT_BLOB = 128  # EIP-7594
FIELD_ELEMENTS_PER_CELL = 64
BYTES_PER_CELL = 2048
_HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------
# error types (src/blob.rs:6-10, src/bls.rs:21-50, src/kzg/mod.rs:15-31)
# ---------------------------------------------------------------------------
class BlobError(Exception):
    def __init__(self, kind: str):
        super().__init__("blob::Error::" + kind)
        self.kind = kind


class FiniteFieldError(Exception):
    def __init__(self, kind: str):
        super().__init__("bls::FiniteFieldError::" + kind)
        self.kind = kind


class ECGroupError(Exception):
    def __init__(self, kind: str):
        super().__init__("bls::ECGroupError::" + kind)
        self.kind = kind


class BlsError(Exception):
    """`bls::Error` -- wraps FiniteField / ECGroup."""

    def __init__(self, inner: Exception):
        super().__init__(str(inner))
        self.inner = inner


class KzgError(Exception):
    """`kzg::Error` -- `Blob(blob::Error)` or `Bls(bls::Error)`."""

    def __init__(self, inner: Exception):
        super().__init__(str(inner))
        self.inner = inner


class LoadSetupError(Exception):
    pass


class CellsError(Exception):
    """rejections of `recover_cells`, of a cell index in `verify_cell_proof_batch` and of a commitment index in its row-indexed form
    (EIP-7594); the reference has no counterpart."""

    def __init__(self, kind: str):
        super().__init__("cells::Error::" + kind)
        self.kind = kind


class EngineError(RuntimeError):
    """negative return from the C ABI: HIP / argument / device failure."""


_STATUS = {
    1: lambda: BlobError("InvalidLen"),
    2: lambda: BlobError("InvalidFieldElement"),
    3: lambda: ECGroupError("InvalidEncoding"),
    4: lambda: ECGroupError("NotOnCurve"),
    5: lambda: ECGroupError("NotInGroup"),
    6: lambda: FiniteFieldError("InvalidEncoding"),
    7: lambda: FiniteFieldError("NotInFiniteField"),
    8: lambda: CellsError("NotEnoughCells"),
    9: lambda: CellsError("Inconsistent"),
    10: lambda: CellsError("CellIndex"),
    11: lambda: CellsError("CommitmentIndex"),
}


def error_from_status(code: int) -> Exception:
    return _STATUS[code]()


def _kzg_error(code: int) -> KzgError:
    inner = error_from_status(code)
    return KzgError(inner if isinstance(inner, BlobError) else BlsError(inner))


def _cell_verify_error(code: int) -> Exception:
    """verify_cell_proof_batch[_rows]'s rejections: CellsError for a cell or commitment index, KzgError for a commitment, a cell or a proof"""
    inner = error_from_status(code)
    return inner if isinstance(inner, CellsError) else _kzg_error(code)


# ---------------------------------------------------------------------------
# library loading -- fails loudly, no fallback
# ---------------------------------------------------------------------------
class _Config(ctypes.Structure):
    """kzg_config (include/kateth_amd.h)"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("window_bits", ctypes.c_int32), ("flags", ctypes.c_int32), ("plane_groups", ctypes.c_int32),
                ("table_budget_bytes", ctypes.c_uint64), ("devices", ctypes.POINTER(ctypes.c_int32)), ("ndev", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    @classmethod
    def new(cls, device=0, window_bits=0, flags=0, plane_groups=0, table_budget_bytes=0, devices=None, ndev=0, reserved=0):
        """KZG_CONFIG_INIT + fields: struct_size = sizeof(kzg_config), which the library checks"""
        return cls(ctypes.sizeof(cls), device, window_bits, flags, plane_groups, table_budget_bytes, devices, ndev, reserved)


CFG_TABLE_MAX = 0x1    # KZG_CFG_TABLE_MAX: the automatic table choice may take the largest table the device has room for (192 GiB)
CFG_BUILD_ASYNC = 0x2  # KZG_CFG_BUILD_ASYNC: usable on a small first-use table at once, the chosen table is built in the background
ALL_DEVICES = 0xFFFFFFFF  # KZG_ALL_DEVICES


def library_path() -> str:
    return os.environ.get("KATETH_AMD_LIB", os.path.join(_HERE, "libkateth_amd.so"))


_LIB = None
_ALT_LIBS = {}

_u8p = ctypes.c_void_p
_i32p = ctypes.POINTER(ctypes.c_int32)
_vpp = ctypes.POINTER(ctypes.c_void_p)
_u64p = ctypes.POINTER(ctypes.c_uint64)

_SIGNATURES = {
    "kzg_last_error": (ctypes.c_char_p, []),
    "kzg_last_error_code": (ctypes.c_int32, []),
    "kzg_ctx_create": (ctypes.c_int32, [_u8p, _u8p, ctypes.POINTER(_Config), ctypes.POINTER(ctypes.c_void_p)]),
    "kzg_ctx_create_multi": (ctypes.c_int32, [_u8p, _u8p, ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32, ctypes.POINTER(_Config), ctypes.POINTER(ctypes.c_void_p)]),
    "kzg_ctx_destroy": (None, [ctypes.c_void_p]),
    "kzg_device_count": (ctypes.c_int32, []),
    "kzg_ctx_members": (ctypes.c_uint32, [ctypes.c_void_p]),
    "kzg_ctx_member_device": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32]),
    "kzg_ctx_member": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_uint32]),
    "kzg_ctx_ready": (ctypes.c_int32, [ctypes.c_void_p]),
    "kzg_ctx_wait_ready": (ctypes.c_int32, [ctypes.c_void_p]),
    "kzg_ctx_window_bits": (ctypes.c_int32, [ctypes.c_void_p]),
    "kzg_ctx_msm_kernel_name": (ctypes.c_char_p, [ctypes.c_void_p]),
    "kzg_ctx_plane_groups": (ctypes.c_int32, [ctypes.c_void_p]),
    "kzg_ctx_table_bytes": (ctypes.c_uint64, [ctypes.c_void_p]),
    "kzg_ctx_comb_balance": (ctypes.c_int32, [ctypes.c_void_p, _u64p]),
    "kzg_blob_to_commitment_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p, _i32p]),
    "kzg_blob_to_commitment_batch_dev": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kzg_blob_to_commitment_batch_affine": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p, _i32p]),
    "kzg_compute_blob_proof_batch_affine": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p]),
    "kzg_compute_proof_batch_affine": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, _u8p, _u8p, _i32p]),
    "kzg_compute_blob_proof_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p]),
    "kzg_compute_blob_proof_batch_dev": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kzg_blob_sidecar_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p, _u8p, _u8p, _i32p]),
    "kzg_blob_sidecar_batch_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kzg_compute_cells_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p, _i32p]),
    "kzg_compute_cells_batch_dev": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "kzg_recover_cells_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p]),
    "kzg_recover_cells_batch_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kzg_compute_cells_and_proofs_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p, _u8p, _i32p]),
    "kzg_compute_cells_and_proofs_batch_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kzg_recover_cells_and_proofs_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, _u8p, _u8p, _i32p]),
    "kzg_recover_cells_and_proofs_batch_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kzg_compute_cells_and_proofs_select_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, _u8p, _u8p, _i32p]),
    "kzg_compute_cells_and_proofs_select_batch_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, _u8p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kzg_recover_cells_and_proofs_select_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint64, _u8p, _u8p, _i32p]),
    "kzg_recover_cells_and_proofs_select_batch_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _u8p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kzg_ctx_cellproof_vectors": (ctypes.c_uint64, [ctypes.c_void_p]),
    "kzg_compute_data_columns_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p, _u8p, _u8p, _i32p]),
    "kzg_compute_data_columns_batch_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kzg_recover_data_columns_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint64, _u8p, _u8p, _i32p]),
    "kzg_recover_data_columns_batch_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    ),
    "kzg_compute_proof_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, _u8p, _u8p, _i32p]),
    "kzg_verify_blob_proof_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint64, _i32p]),
    "kzg_verify_blob_proof_batch_dev": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _i32p, ctypes.c_void_p]),
    "kzg_verify_blob_proof": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, _i32p]),
    "kzg_verify_proof": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, _u8p, _i32p]),
    "kzg_verify_proof_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint64, _i32p]),
    "kzg_verify_proof_batch_dev": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _i32p, ctypes.c_void_p]),
    "kzg_verify_cell_proof_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u64p, _u8p, _u8p, ctypes.c_uint64, _i32p]),
    "kzg_verify_cell_proof_batch_dev": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _i32p, ctypes.c_void_p]),
    "kzg_ctx_g1_monomial": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, _u8p]),
    "kzg_verify_proof_batch_group_dev": (ctypes.c_int32, [ctypes.c_void_p, _vpp, _vpp, _vpp, _vpp, _u64p, _i32p, _vpp]),
    "kzg_verify_proof_phase1_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u8p, _i32p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p],
    ),
    "kzg_verify_blob_proof_batch_each": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p, _i32p]),
    "kzg_verify_blob_proof_batch_each_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u8p, _i32p, _i32p, ctypes.c_void_p],
    ),
    "kzg_verify_proof_batch_each": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p, _i32p]),
    "kzg_verify_proof_batch_each_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u8p, _i32p, _i32p, ctypes.c_void_p],
    ),
    "kzg_verify_cell_proof_batch_rows": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u64p, _u64p, _u8p, _u8p, ctypes.c_uint64, _i32p]),
    "kzg_verify_cell_proof_batch_rows_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _i32p, ctypes.c_void_p]),
    "kzg_verify_cell_proof_batch_rows_each": (
        ctypes.c_int32,
        [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u64p, _u64p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p, _i32p, _i32p]),
    "kzg_verify_cell_proof_batch_rows_each_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u8p, _i32p,
         _i32p, _i32p, ctypes.c_void_p]),
    "kzg_cell_row_weights": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u64p, ctypes.c_uint64, ctypes.c_uint64, _u8p]),
    "kzg_verify_blob_cell_proofs_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint64, _i32p]),
    "kzg_verify_blob_cell_proofs_batch_dev": (
        ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _i32p, ctypes.c_void_p]),
    "kzg_verify_blob_cell_proofs_batch_each": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p, _i32p]),
    "kzg_verify_blob_cell_proofs_batch_each_dev": (
        ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u8p, _i32p, _i32p, ctypes.c_void_p]),
    "kzg_blob_cell_weights": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, ctypes.c_uint64, _u8p]),
    "kzg_verify_cell_proof_batch_each": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u64p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p, _i32p]),
    "kzg_verify_cell_proof_batch_each_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u8p, _i32p, _i32p, ctypes.c_void_p],
    ),
    "kzg_g1_monomial_lincomb": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p]),
    "kzg_verify_each_checks": (ctypes.c_uint64, [ctypes.c_void_p]),
    "kzg_ctx_sessions_created": (ctypes.c_uint64, [ctypes.c_void_p]),
    "kzg_verify_session_tree": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]),
    "kzg_verify_session_tree_range": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, _u8p]),
    "kzg_g1_decompress_batch": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _u8p, _i32p]),
    "kzg_evaluate_blobs": (ctypes.c_int32, [ctypes.c_void_p, _u8p, _u8p, ctypes.c_uint64, _u8p, _i32p]),
    "kzg_verify_phase1_dev": (
        ctypes.c_int32,
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, _u8p, _i32p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p],
    ),
    "kzg_blob_to_commitment_batch_group_dev": (ctypes.c_int32, [ctypes.c_void_p, _vpp, _u64p, _vpp, _vpp, _vpp]),
    "kzg_compute_blob_proof_batch_group_dev": (ctypes.c_int32, [ctypes.c_void_p, _vpp, _vpp, _u64p, _vpp, _vpp, _vpp]),
    "kzg_verify_blob_proof_batch_group_dev": (ctypes.c_int32, [ctypes.c_void_p, _vpp, _vpp, _vpp, _u64p, _i32p, _vpp]),
    "kzg_recommended_env": (ctypes.c_char_p, []),
    "kzg_ctx_workspace_bytes": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint32]),
    "kzg_verify_phase2_dev": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _u8p]),
    "kzg_verify_session_destroy": (None, [ctypes.c_void_p]),
    "kzg_verify_session_zy": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, _u8p, _u8p]),
    "kzg_verify_batch_finish": (ctypes.c_int32, [ctypes.c_void_p, _u8p, ctypes.c_uint64, _i32p]),
    "kzg_synth_blobs_dev": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]),
    "kzg_profile_begin": (ctypes.c_int32, [ctypes.c_void_p]),
    "kzg_profile_end": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]),
    "kzg_profile_end_kinds": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]),
    "kzg_profile_kind_name": (ctypes.c_char_p, [ctypes.c_int32]),
    "kzg_ctx_adds_per_blob": (ctypes.c_uint64, [ctypes.c_void_p]),
    "kzg_selftest_field_mul": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "kzg_selftest_exception_guard": (ctypes.c_int32, [ctypes.c_int32]),
    "kzg_microbench_fp_mul": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_float)]),
    "kzg_clock_probe_launch": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32]),
    "kzg_clock_probe_read": (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "kzg_microbench_valu_issue": (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _ensure_hip_runtime():
    """libkateth_amd.so carries no DT_NEEDED for the HIP runtime: it binds to the
    libamdhip64 already in the process.  PyTorch-ROCm wheels bundle their own copy
    and a second runtime in the same process breaks both, so when torch is
    installed its runtime is the one that gets loaded (and promoted to the global
    symbol scope); otherwise the system ROCm runtime is."""
    mode = getattr(ctypes, "RTLD_GLOBAL", 0)
    try:
        import torch  # noqa: F401  (plumbing only: loads torch's HIP runtime)

        cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=mode)
            return
    except ImportError:
        pass
    for cand in (os.environ.get("KATETH_AMD_HIP_RUNTIME", ""), "/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"):
        if cand:
            try:
                ctypes.CDLL(cand, mode=mode)
                return
            except OSError:
                continue
    raise ImportError("kateth_amd: no HIP runtime (libamdhip64.so) could be loaded")


def load_library(path: Optional[str] = None):
    """dlopen the HIP engine.  Raises if it has not been built -- by design there
    is nothing to fall back to.  `path`: another build of the same C ABI (the tests'
    cross-check build under tests/radix32); the default is the product library."""
    global _LIB
    if path is None and _LIB is not None:
        return _LIB
    if path is not None and path in _ALT_LIBS:
        return _ALT_LIBS[path]
    alt = path is not None
    path = path or library_path()
    if not os.path.exists(path):
        raise ImportError(
            "kateth_amd: HIP engine %s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % path
        )
    _ensure_hip_runtime()
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export what include/kateth_amd.h declares
        fn.restype = restype
        fn.argtypes = argtypes
    if alt:
        _ALT_LIBS[path] = lib
    else:
        _LIB = lib
    return lib


def _buf(data) -> bytes:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    if hasattr(data, "to_bytes") and not isinstance(data, int):  # a Blob
        return data.to_bytes()
    return bytes(bytearray(data))


def versioned_hash(commitment48) -> bytes:
    """EIP-4844's `kzg_to_versioned_hash`: 0x01 || SHA-256(commitment48)[1:32], on the host (hashlib; no GPU, no library)."""
    import hashlib

    commitment48 = _buf(commitment48)
    if len(commitment48) != 48:
        raise ValueError("a commitment is 48 bytes")
    return b"\x01" + hashlib.sha256(commitment48).digest()[1:]


def _has_noncanonical_element(blob: bytes) -> bool:
    """Blob::from_slice's per-element check (src/blob.rs:32-34 -> src/bls.rs:110-120): some 32-byte big-endian element >= r.
    Host side, error path only: the mirror needs it to name the FIRST failing blob when a later one has the wrong length."""
    r = _R.to_bytes(32, "big")
    return any(blob[k:k + 32] >= r for k in range(0, len(blob) - len(blob) % 32, 32))


def _unhex(s: str) -> bytes:
    """`Bytes` deserialiser (src/bytes.rs:30-37): optional 0x prefix."""
    return bytes.fromhex(s[2:] if s.startswith("0x") else s)


_R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # Fr modulus
_P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB  # Fp modulus


class Blob:
    """`Blob<4096>` (src/blob.rs:18-76): a validated 131,072-byte blob.  Host-side container only -- every computation
    on it happens in the engine; `from_slice` repeats the reference's parse checks so that the type has its meaning."""

    BYTES = BYTES_PER_BLOB  # Blob::<4096>::BYTES, src/blob.rs:24

    def __init__(self, data: bytes):
        self._data = data

    @classmethod
    def from_slice(cls, data) -> "Blob":
        """src/blob.rs:26-37: InvalidLen unless 131,072 bytes; InvalidFieldElement unless every 32-byte big-endian chunk is < r."""
        data = _buf(data)
        if len(data) != cls.BYTES:
            raise BlobError("InvalidLen")
        rb = _R.to_bytes(32, "big")
        for i in range(0, cls.BYTES, 32):
            if data[i:i + 32] >= rb:  # big-endian: bytewise order is numeric order
                raise BlobError("InvalidFieldElement")
        return cls(data)

    def to_bytes(self) -> bytes:
        """src/blob.rs:39-46"""
        return self._data

    @classmethod
    def random(cls, gen) -> "Blob":
        """src/blob.rs:66-76: each element = SHA-256(512 bytes from `gen`) reduced mod r (`Fr::hash_to`, src/bls.rs:189-205).
        `gen` is anything with randbytes(n) (random.Random) or a callable n -> bytes."""
        import hashlib

        fill = gen.randbytes if hasattr(gen, "randbytes") else gen
        out = bytearray()
        for _ in range(cls.BYTES // 32):
            out += (int.from_bytes(hashlib.sha256(fill(512)).digest(), "big") % _R).to_bytes(32, "big")
        return cls(bytes(out))

    def __bytes__(self):
        return self._data

    def __len__(self):
        return len(self._data)


class P1:
    """`bls::P1` as the reference's producers return it (`Commitment = Proof = P1`, src/kzg/mod.rs:9-10): the engine hands
    the point over as a 96-byte blst_p1_affine image (x || y, little-endian limbs of the 2^384-Montgomery residue; all
    zero = infinity), which is what a Rust caller feeds to blst_p1_from_affine.  `compress` is the caller-side
    `Compress::compress` (src/bls.rs:491-503, a blst CPU call in the reference): a change of encoding of a point the GPU
    already normalised, kept here so the mirror's call sites read like benches/kzg.rs:24-32."""

    COMPRESSED = 48

    def __init__(self, affine96: bytes):
        assert len(affine96) == 96
        self.affine = bytes(affine96)

    def is_inf(self) -> bool:
        return not any(self.affine)

    def compress(self) -> bytes:
        if self.is_inf():
            return bytes([0xC0]) + bytes(47)
        rinv = pow(1 << 384, -1, _P)
        x = int.from_bytes(self.affine[:48], "little") * rinv % _P
        y = int.from_bytes(self.affine[48:], "little") * rinv % _P
        out = bytearray(x.to_bytes(48, "big"))
        out[0] |= 0x80 | (0x20 if y > (_P - 1) // 2 else 0)
        return bytes(out)

    def __eq__(self, other):
        return isinstance(other, P1) and self.affine == other.affine

    def __hash__(self):
        return hash(self.affine)


class Setup:
    """`Setup<4096, 65>` (src/kzg/setup.rs:37-42) resident on one MI355X."""

    G1 = 4096
    G2 = 65

    def __init__(self, handle: int, lib):
        self._h = ctypes.c_void_p(handle)
        self._lib = lib

    # -- construction --------------------------------------------------------
    @classmethod
    def load_json(cls, path, device: int = 0, window_bits: int = 0, lib_path: Optional[str] = None, plane_groups: int = 0, devices=None,
                  table_max: bool = False, build_async: bool = False, table_budget_bytes: int = 0) -> "Setup":
        """`Setup::load_json` (src/kzg/setup.rs:46-82).  window_bits = 0: the engine picks the fastest table class within the
        budget (default 100 GiB -> the 96-GiB table; `table_max` lifts the cap -> 192 GiB on an idle MI355X) that the device
        has room for (include/kateth_amd.h, kzg_config).  `devices`: a list of HIP ordinals, or "all" -- a GROUP context whose
        host-buffer methods shard every batch over the listed GPUs.  `build_async`: return as soon as a small first-use table
        stands; the chosen table is built in the background (`ready`, `wait_ready`)."""
        try:
            with open(path) as fh:
                raw = json.load(fh)
        except OSError as err:
            raise LoadSetupError("Io(%s)" % err)
        except ValueError as err:
            raise LoadSetupError("Serde(%s)" % err)
        try:
            g1 = [_unhex(s) for s in raw["g1_lagrange"]]
            g2 = [_unhex(s) for s in raw["g2_monomial"]]
        except (KeyError, ValueError, AttributeError) as err:
            raise LoadSetupError("Serde(%s)" % err)
        return cls.from_bytes(g1, g2, device=device, window_bits=window_bits, lib_path=lib_path, plane_groups=plane_groups, devices=devices,
                              table_max=table_max, build_async=build_async, table_budget_bytes=table_budget_bytes)

    @classmethod
    def from_bytes(cls, g1_lagrange: Sequence[bytes], g2_monomial: Sequence[bytes], device: int = 0, window_bits: int = 0,
                   lib_path: Optional[str] = None, plane_groups: int = 0, devices=None, table_max: bool = False, build_async: bool = False,
                   table_budget_bytes: int = 0) -> "Setup":
        if len(g1_lagrange) != cls.G1:
            raise LoadSetupError("InvalidLenG1Lagrange")  # src/kzg/setup.rs:52-54
        if len(g2_monomial) != cls.G2:
            raise LoadSetupError("InvalidLenG2Monomial")  # src/kzg/setup.rs:55-57
        if any(len(p) != 48 for p in g1_lagrange) or any(len(p) != 96 for p in g2_monomial):
            raise LoadSetupError("Bls(ECGroup(InvalidEncoding))")
        lib = load_library(lib_path)
        flags = (CFG_TABLE_MAX if table_max else 0) | (CFG_BUILD_ASYNC if build_async else 0)
        cfg = _Config.new(device, window_bits, flags, plane_groups, table_budget_bytes, None, 0, 0)
        keep = None
        if devices is not None:
            if isinstance(devices, str):
                assert devices == "all", devices
                cfg.ndev = ALL_DEVICES
            else:
                keep = (ctypes.c_int32 * len(devices))(*devices)
                cfg.devices = ctypes.cast(keep, ctypes.POINTER(ctypes.c_int32))
                cfg.ndev = len(devices)
        out = ctypes.c_void_p()
        rc = lib.kzg_ctx_create(b"".join(g1_lagrange), b"".join(g2_monomial), ctypes.byref(cfg), ctypes.byref(out))
        if rc in (-4, -5):  # LoadSetupError::Bls(bls::Error::ECGroup(..)), src/kzg/setup.rs:59-72
            code = lib.kzg_last_error_code()
            kind = str(error_from_status(code)) if code in _STATUS else "ECGroup"
            raise LoadSetupError("Bls(%s): %s" % (kind, lib.kzg_last_error().decode()))
        if rc == -6:  # no counterpart in the reference: a setup whose points cancel within a comb block (include/kateth_amd.h)
            raise LoadSetupError("Unsupported: %s" % lib.kzg_last_error().decode())
        if rc != 0:
            raise EngineError("kzg_ctx_create failed (%d): %s" % (rc, lib.kzg_last_error().decode()))
        return cls(out.value, lib)

    # -- group contexts / background build ------------------------------------
    @property
    def members(self) -> int:
        """devices this context shards host-buffer batches over (1 = a single-device context)"""
        return self._lib.kzg_ctx_members(self._h)

    def member_device(self, k: int) -> int:
        return self._lib.kzg_ctx_member_device(self._h, k)

    def member(self, k: int) -> "Setup":
        """member k as a single-device Setup (borrowed: it lives as long as this context; close() on it is a no-op)"""
        h = self._lib.kzg_ctx_member(self._h, k)
        if not h:
            raise IndexError(k)
        m = Setup(h, self._lib)
        m._borrowed = True
        m._owner = self
        return m

    @property
    def ready(self) -> bool:
        return bool(self._lib.kzg_ctx_ready(self._h))

    def wait_ready(self):
        self._check(self._lib.kzg_ctx_wait_ready(self._h), "kzg_ctx_wait_ready")

    def close(self):
        if self._h:
            if not getattr(self, "_borrowed", False):
                self._lib.kzg_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> int:
        return self._h.value

    @property
    def window_bits(self) -> int:
        return self._lib.kzg_ctx_window_bits(self._h)

    @property
    def plane_groups(self) -> int:
        return self._lib.kzg_ctx_plane_groups(self._h)

    @property
    def msm_kernel_name(self) -> str:
        return self._lib.kzg_ctx_msm_kernel_name(self._h).decode()

    @property
    def table_bytes(self) -> int:
        return self._lib.kzg_ctx_table_bytes(self._h)

    def workspace_bytes(self):
        """bytes of the three commitment / proof workspace slots as allocated so far"""
        return [int(self._lib.kzg_ctx_workspace_bytes(self._h, k)) for k in range(3)]

    def comb_balance(self) -> dict:
        """the balance plan of the two-blobs-per-wave MSM launches and the newest timing record taken (kzg_ctx_comb_balance)"""
        w = (ctypes.c_uint64 * 44)()
        self._check(self._lib.kzg_ctx_comb_balance(self._h, w), "kzg_ctx_comb_balance")
        w = [int(x) for x in w]
        rec = None
        if w[16]:
            rec = {"seq": w[16], "start": w[17], "end": w[18:26], "end_us": [(e - w[17]) / 100.0 for e in w[18:26]], "units": w[27],
                   "ran": {"partner": w[28:36], "shed": w[36:44]}}
        return {"partner": w[0:8], "shed": w[8:16], "record": rec}

    def _check(self, rc: int, what: str):
        if rc < 0:
            raise EngineError("%s failed (%d): %s" % (what, rc, self._lib.kzg_last_error().decode()))

    def _verdict(self, what: str, args, tail=(), to_error=_kzg_error) -> bool:
        """a boolean verification call `what`(handle, *args, &ok, *tail): EngineError when the engine failed, to_error(code) for a rejected
        input, else the verdict"""
        ok = ctypes.c_int32(0)
        rc = getattr(self._lib, what)(self._h, *args, ctypes.byref(ok), *tail)
        self._check(rc, what)
        if rc > 0:
            raise to_error(rc)
        return bool(ok.value)

    def _verdicts(self, what: str, args, n: int, tail=()) -> Tuple[List[bool], List[int], bool]:
        """a per-item verification call `what`(handle, *args, n, ok_each, status, &ok, *tail) -> (ok_each, status, ok)"""
        ok_each, status, ok = ctypes.create_string_buffer(max(n, 1)), (ctypes.c_int32 * max(n, 1))(), ctypes.c_int32(0)
        rc = getattr(self._lib, what)(self._h, *args, n, ctypes.cast(ok_each, _u8p), status, ctypes.byref(ok), *tail)
        self._check(rc, what)
        if rc > 0:  # the ABI reports rejected items in status[], never as the call's code
            raise EngineError("%s returned %d" % (what, rc))
        return [bool(b) for b in ok_each.raw[:n]], list(status[:n]), bool(ok.value)

    def _produce(self, what: str, inputs, n: int, out_bytes):
        """a host-buffer producer call `what`(handle, *inputs, n, *outputs, status) -> (output, ..., [status]).  `out_bytes`: bytes per item of
        every output, None for one the caller does not want (a null pointer goes down, None comes back)"""
        outs = [None if b is None else ctypes.create_string_buffer(b * n) for b in out_bytes]
        status = (ctypes.c_int32 * n)()
        rc = getattr(self._lib, what)(self._h, *inputs, n, *[None if o is None else ctypes.cast(o, ctypes.c_void_p) for o in outs], status)
        self._check(rc, what)
        return tuple(None if o is None else o.raw for o in outs) + (list(status),)

    @staticmethod
    def _host_args(*buffers):
        """contiguous host inputs: bytes-like objects, or raw host addresses (ints) passed through"""
        return [a if isinstance(a, int) else _buf(a) for a in buffers]

    @staticmethod
    def _cell_index_array(cell_indices, n: int):
        """n cell indices for the C ABI: a sequence of ints, a bytes-like object of n native uint64, or a raw host address"""
        if isinstance(cell_indices, int):
            return ctypes.cast(cell_indices, _u64p)
        if isinstance(cell_indices, (bytes, bytearray, memoryview)):
            return (ctypes.c_uint64 * n).from_buffer_copy(cell_indices)
        return (ctypes.c_uint64 * n)(*cell_indices)

    # -- batch entry points (host buffers) --------------------------------------
    def blob_to_commitment_batch(self, blobs: bytes, n: Optional[int] = None):
        """n concatenated blobs -> (n*48 bytes, [status])."""
        blobs = _buf(blobs)
        n = len(blobs) // BYTES_PER_BLOB if n is None else n
        if len(blobs) != n * BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        return self._produce("kzg_blob_to_commitment_batch", [blobs], n, [48])

    def compute_blob_proof_batch(self, blobs: bytes, commitments: bytes):
        blobs, commitments = _buf(blobs), _buf(commitments)
        n = len(commitments) // 48
        if len(blobs) != n * BYTES_PER_BLOB or len(commitments) != 48 * n:
            raise BlobError("InvalidLen")
        return self._produce("kzg_compute_blob_proof_batch", [blobs, commitments], n, [48])

    def blob_sidecar_batch(self, blobs: bytes, n: Optional[int] = None):
        """n concatenated blobs -> (n*48 bytes of commitments, n*48 bytes of blob proofs, n*32 bytes of versioned hashes, [status]):
        `blob_to_commitment`, then `blob_proof` on the same blob, then EIP-4844's `kzg_to_versioned_hash`, the blobs uploaded once."""
        blobs = _buf(blobs)
        n = len(blobs) // BYTES_PER_BLOB if n is None else n
        if len(blobs) != n * BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        return self._produce("kzg_blob_sidecar_batch", [blobs], n, [48, 48, 32])

    def compute_cells_batch(self, blobs: bytes, n: Optional[int] = None):
        """n concatenated blobs -> (n * 128 * 2048 bytes of cells, [status]): EIP-7594's `compute_cells` per blob.  Cells 0..63 of an
        accepted blob are the blob itself; a rejected blob gets zero bytes."""
        blobs = _buf(blobs)
        n = len(blobs) // BYTES_PER_BLOB if n is None else n
        if len(blobs) != n * BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        return self._produce("kzg_compute_cells_batch", [blobs], n, [CELLS_PER_EXT_BLOB * BYTES_PER_CELL])

    def recover_cells_batch(self, cells: bytes, present: bytes, n: Optional[int] = None):
        """n cell sets (128 * 2048 bytes each, laid out like `compute_cells_batch`'s output) and n 16-byte masks (cell c present iff bit
        c & 7 of byte c >> 3) -> (n * 128 * 2048 bytes of cells, [status]).  Absent cells may hold anything.  Status 8: fewer than 64
        cells present; 2: a present element >= r; 9: the present cells do not lie on one polynomial of degree < 4096 (a check the spec
        does not make).  A rejected item gets zero bytes."""
        cells, present = _buf(cells), _buf(present)
        n = len(present) // 16 if n is None else n
        if len(cells) != n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL or len(present) != n * 16:
            raise ValueError("recover_cells_batch: n * 262144 bytes of cells and n * 16 bytes of mask")
        return self._produce("kzg_recover_cells_batch", [cells, present], n, [CELLS_PER_EXT_BLOB * BYTES_PER_CELL])

    def compute_cells_and_proofs_batch(self, blobs: bytes, n: Optional[int] = None, want_cells: bool = True):
        """n concatenated blobs -> (n * 128 * 2048 bytes of cells, or None without `want_cells`; n * 128 * 48 bytes of cell proofs;
        [status]): EIP-7594's `compute_cells_and_kzg_proofs` per blob.  Proof k of blob i is at byte 48 * (128 i + k).  A rejected blob
        gets zero bytes for both."""
        blobs = _buf(blobs)
        n = len(blobs) // BYTES_PER_BLOB if n is None else n
        if len(blobs) != n * BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        return self._produce("kzg_compute_cells_and_proofs_batch", [blobs], n,
                             [CELLS_PER_EXT_BLOB * BYTES_PER_CELL if want_cells else None, CELLS_PER_EXT_BLOB * 48])

    def recover_cells_and_proofs_batch(self, cells: bytes, present: bytes, n: Optional[int] = None):
        """`recover_cells_batch` with the 128 cell proofs of every item: -> (n * 128 * 2048 bytes of cells, n * 128 * 48 bytes of proofs,
        [status]).  Statuses as `recover_cells_batch`; a rejected item gets zero bytes for both."""
        cells, present = _buf(cells), _buf(present)
        n = len(present) // 16 if n is None else n
        if len(cells) != n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL or len(present) != n * 16:
            raise ValueError("recover_cells_and_proofs_batch: n * 262144 bytes of cells and n * 16 bytes of mask")
        return self._produce("kzg_recover_cells_and_proofs_batch", [cells, present], n, [CELLS_PER_EXT_BLOB * BYTES_PER_CELL, CELLS_PER_EXT_BLOB * 48])

    def _select_call(self, what: str, inputs, n: int, proofs, want_cells: bool):
        """a select call `what`(handle, *inputs, n, out_cells, inout_proofs, status): the proof buffer starts as `proofs` (zero bytes when None)"""
        size = n * CELLS_PER_EXT_BLOB * 48
        if proofs is not None and len(_buf(proofs)) != size:
            raise ValueError("%s: the proof buffer is n * 6144 bytes" % what)
        io = ctypes.create_string_buffer(bytes(_buf(proofs)) if proofs is not None else bytes(size), size)
        cells = ctypes.create_string_buffer(n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if want_cells else None
        status = (ctypes.c_int32 * n)()
        rc = getattr(self._lib, what)(self._h, *inputs, n, None if cells is None else ctypes.cast(cells, ctypes.c_void_p), ctypes.cast(io, ctypes.c_void_p), status)
        self._check(rc, what)
        return (None if cells is None else cells.raw), io.raw, list(status)

    def compute_cells_and_proofs_select_batch(self, blobs: bytes, want: bytes, proofs: Optional[bytes] = None, want_cells: bool = True):
        """`compute_cells_and_proofs_batch` for CHOSEN cells: `want` is n 16-byte masks (cell c wanted iff bit c & 7 of byte c >> 3) ->
        (cells or None, n * 128 * 48 bytes of proofs, [status]).  The wanted proofs stand where the full call puts them; every other
        position keeps the bytes of `proofs` (zero bytes when None).  A rejected blob's wanted positions are zero bytes."""
        blobs, want = _buf(blobs), _buf(want)
        n = len(want) // 16
        if len(blobs) != n * BYTES_PER_BLOB or len(want) != n * 16:
            raise ValueError("compute_cells_and_proofs_select_batch: n * 131072 bytes of blobs and n * 16 bytes of mask")
        return self._select_call("kzg_compute_cells_and_proofs_select_batch", [blobs, want], n, proofs, want_cells)

    def recover_cells_and_proofs_select_batch(self, cells: bytes, present: bytes, want: bytes, proofs: Optional[bytes] = None):
        """`recover_cells_and_proofs_batch` for CHOSEN cells: `want` as in `compute_cells_and_proofs_select_batch`, independent of
        `present` -> (cells, proofs, [status]).  A node passes the proofs it received in `proofs` and wants the absent cells'."""
        cells, present, want = _buf(cells), _buf(present), _buf(want)
        n = len(present) // 16
        if len(cells) != n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL or len(present) != n * 16 or len(want) != n * 16:
            raise ValueError("recover_cells_and_proofs_select_batch: n * 262144 bytes of cells and two n * 16 bytes of masks")
        return self._select_call("kzg_recover_cells_and_proofs_select_batch", [cells, present, want], n, proofs, True)

    # -- data columns: cells and proofs as COLUMN MATRICES of n rows -- the cell of (column c, row b) at 2048 * (c * n + b), its proof at
    # 48 * (c * n + b) -- so that column c's sidecar payload is one run of bytes
    def compute_data_columns_batch(self, blobs: bytes, n: Optional[int] = None, want_commitments: bool = True):
        """A block's n blobs -> (n * 48 bytes of commitments, or None without `want_commitments`; the column matrix of cells,
        128 * n * 2048 bytes; the column matrix of proofs, 128 * n * 48 bytes; [status]).  Cells, proofs and statuses are
        `compute_cells_and_proofs_batch`'s in the column layout, the commitments `blob_to_commitment_batch`'s; the blobs are uploaded
        once.  A rejected blob's row is zero bytes in every column, and so is its commitment."""
        blobs = _buf(blobs)
        n = len(blobs) // BYTES_PER_BLOB if n is None else n
        if len(blobs) != n * BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        coms = ctypes.create_string_buffer(n * 48) if want_commitments else None
        cells = ctypes.create_string_buffer(n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL)
        proofs = ctypes.create_string_buffer(n * CELLS_PER_EXT_BLOB * 48)
        status = (ctypes.c_int32 * max(n, 1))()
        rc = self._lib.kzg_compute_data_columns_batch(self._h, blobs, n, None if coms is None else ctypes.cast(coms, _u8p), ctypes.cast(cells, _u8p),
                                                      ctypes.cast(proofs, _u8p), status)
        self._check(rc, "kzg_compute_data_columns_batch")
        return (None if coms is None else coms.raw), cells.raw, proofs.raw, list(status[:n])

    def recover_data_columns_batch(self, column_cells: bytes, present: bytes, want: Optional[bytes] = None, n: Optional[int] = None,
                                   proofs: Optional[bytes] = None):
        """The column matrix of cells of n rows with the columns of the ONE 16-byte mask `present` filled in (absent columns may hold
        anything) -> (the column matrix of all 128 columns, the column matrix of proofs or None, [status]).  `want` is the one mask of
        the columns whose proofs to compute, into a copy of `proofs` (zero bytes when None) whose other positions stay; want = None:
        cells only.  Statuses per row as `recover_cells_batch`; a rejected row is zero bytes in every column."""
        column_cells, present = _buf(column_cells), _buf(present)
        n = len(column_cells) // (CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if n is None else n
        size = n * CELLS_PER_EXT_BLOB * 48
        if len(column_cells) != n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL or len(present) != 16 or (want is not None and len(_buf(want)) != 16):
            raise ValueError("recover_data_columns_batch: n * 262144 bytes of cells and 16-byte masks")
        if proofs is not None and (want is None or len(_buf(proofs)) != size):
            raise ValueError("recover_data_columns_batch: the proof matrix is n * 6144 bytes and goes with `want`")
        out = ctypes.create_string_buffer(n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL)
        io = None if want is None else ctypes.create_string_buffer(bytes(_buf(proofs)) if proofs is not None else bytes(size), size)
        status = (ctypes.c_int32 * max(n, 1))()
        rc = self._lib.kzg_recover_data_columns_batch(self._h, column_cells, present, None if want is None else _buf(want), n, ctypes.cast(out, _u8p),
                                                      None if io is None else ctypes.cast(io, _u8p), status)
        self._check(rc, "kzg_recover_data_columns_batch")
        return out.raw, (None if io is None else io.raw), list(status[:n])

    def data_column_sidecars(self, blobs):
        """The consensus specs' compute_matrix + get_data_column_sidecars for one block: `blobs` (a list of blobs, or their
        concatenation) -> (commitments, columns), `columns` the list of 128 (column_index, cells, proofs) that `verify_data_columns`
        takes, cells and proofs with one entry per blob in the blobs' order.  Raises what `compute_cells` raises for a rejected blob."""
        blobs = b"".join(bytes(_buf(b)) for b in blobs) if isinstance(blobs, (list, tuple)) else _buf(blobs)
        if len(blobs) % BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        n = len(blobs) // BYTES_PER_BLOB
        coms, cells, proofs, status = self.compute_data_columns_batch(blobs, n)
        for code in status:
            if code:
                raise error_from_status(code)
        return [coms[48 * b:48 * (b + 1)] for b in range(n)], self._column_lists(n, range(CELLS_PER_EXT_BLOB), cells, proofs)

    @staticmethod
    def _column_lists(n, column_indices, cells, proofs):
        """column matrices -> [(column_index, [n cells], [n proofs])] for the columns named"""
        return [(c, [cells[BYTES_PER_CELL * (c * n + b):BYTES_PER_CELL * (c * n + b + 1)] for b in range(n)],
                 [proofs[48 * (c * n + b):48 * (c * n + b + 1)] for b in range(n)]) for c in column_indices]

    def recover_data_columns(self, n_rows: int, columns):
        """The consensus specs' recover_matrix for one block, with the proofs: at least 64 column sidecars (column_index, cells,
        proofs) of n_rows rows each, in any order -> all 128, in column order.  The given columns come back as they came and only the
        absent columns' proofs are computed.  ValueError for a malformed list; BlobError / CellsError as `recover_cells` for a row that
        cannot be recovered."""
        n, columns = int(n_rows), list(columns)
        seen = sorted(int(c) for c, _, _ in columns)
        if any(not 0 <= c < CELLS_PER_EXT_BLOB for c in seen) or any(a == b for a, b in zip(seen, seen[1:])):
            raise ValueError("recover_data_columns: column indices are distinct and below 128")
        if len(seen) < CELLS_PER_EXT_BLOB // 2:
            raise ValueError("recover_data_columns: %d columns, need 64..128" % len(seen))
        cells, proofs, mask = bytearray(n * CELLS_PER_EXT_BLOB * BYTES_PER_CELL), bytearray(n * CELLS_PER_EXT_BLOB * 48), bytearray(16)
        for c, col_cells, col_proofs in columns:
            c, col_cells, col_proofs = int(c), [_buf(v) for v in col_cells], [_buf(v) for v in col_proofs]
            if len(col_cells) != n or len(col_proofs) != n or any(len(v) != BYTES_PER_CELL for v in col_cells) or any(len(v) != 48 for v in col_proofs):
                raise ValueError("recover_data_columns: column %d needs %d cells of %d bytes and as many 48-byte proofs" % (c, n, BYTES_PER_CELL))
            cells[BYTES_PER_CELL * c * n:BYTES_PER_CELL * (c + 1) * n] = b"".join(bytes(v) for v in col_cells)
            proofs[48 * c * n:48 * (c + 1) * n] = b"".join(bytes(v) for v in col_proofs)
            mask[c >> 3] |= 1 << (c & 7)
        if n == 0:
            return self._column_lists(0, range(CELLS_PER_EXT_BLOB), b"", b"")
        out, all_proofs, status = self.recover_data_columns_batch(bytes(cells), bytes(mask), bytes(b ^ 0xFF for b in mask), n, bytes(proofs))
        for code in status:
            if code:
                raise error_from_status(code)
        return self._column_lists(n, range(CELLS_PER_EXT_BLOB), out, all_proofs)

    def compute_proof_batch(self, blobs: bytes, zs: bytes):
        blobs, zs = _buf(blobs), _buf(zs)
        n = len(zs) // 32
        if len(blobs) != n * BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        return self._produce("kzg_compute_proof_batch", [blobs, zs], n, [48, 32])

    # -- the same producers returning POINTS (`Commitment = Proof = P1`, src/kzg/mod.rs:9-10) as 96-byte blst_p1_affine images
    def blob_to_commitment_batch_affine(self, blobs: bytes, n: Optional[int] = None):
        blobs = _buf(blobs)
        n = len(blobs) // BYTES_PER_BLOB if n is None else n
        if len(blobs) != n * BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        return self._produce("kzg_blob_to_commitment_batch_affine", [blobs], n, [96])

    def compute_blob_proof_batch_affine(self, blobs: bytes, commitments: bytes):
        blobs, commitments = _buf(blobs), _buf(commitments)
        n = len(commitments) // 48
        if len(blobs) != n * BYTES_PER_BLOB or len(commitments) != 48 * n:
            raise BlobError("InvalidLen")
        return self._produce("kzg_compute_blob_proof_batch_affine", [blobs, commitments], n, [96])

    def compute_proof_batch_affine(self, blobs: bytes, zs: bytes):
        blobs, zs = _buf(blobs), _buf(zs)
        n = len(zs) // 32
        if len(blobs) != n * BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        return self._produce("kzg_compute_proof_batch_affine", [blobs, zs], n, [96, 32])

    # -- reference-shaped API ----------------------------------------------------
    # `Setup::blob_to_commitment / blob_proof / proof` with the reference's return type (a point), for call sites shaped
    # like benches/kzg.rs:24-32 (`kzg.blob_to_commitment(blob).unwrap().compress(&mut bytes)`)
    def blob_to_commitment_point(self, blob) -> P1:
        blob = _buf(blob)
        if len(blob) != BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        out, status = self.blob_to_commitment_batch_affine(blob, 1)
        if status[0]:
            raise error_from_status(status[0])
        return P1(out)

    def blob_proof_point(self, blob, commitment: bytes) -> P1:
        blob, commitment = _buf(blob), _buf(commitment)
        if len(blob) != BYTES_PER_BLOB:
            raise KzgError(BlobError("InvalidLen"))
        if len(commitment) != 48:
            raise KzgError(BlsError(ECGroupError("InvalidEncoding")))
        out, status = self.compute_blob_proof_batch_affine(blob, commitment)
        if status[0]:
            raise _kzg_error(status[0])
        return P1(out)

    def proof_point(self, blob, point: bytes):
        """(P1 proof, y32)"""
        blob, point = _buf(blob), _buf(point)
        if len(blob) != BYTES_PER_BLOB:
            raise KzgError(BlobError("InvalidLen"))
        if len(point) != 32:
            raise KzgError(BlsError(FiniteFieldError("InvalidEncoding")))
        proofs, ys, status = self.compute_proof_batch_affine(blob, point)
        if status[0]:
            raise _kzg_error(status[0])
        return P1(proofs), ys

    def blob_to_commitment(self, blob: bytes) -> bytes:
        """`Setup::blob_to_commitment` + `compress`: 48-byte commitment or BlobError."""
        blob = _buf(blob)
        if len(blob) != BYTES_PER_BLOB:
            raise BlobError("InvalidLen")  # src/blob.rs:27-29
        out, status = self.blob_to_commitment_batch(blob, 1)
        if status[0]:
            raise error_from_status(status[0])
        return out

    def blob_sidecar(self, blob: bytes) -> Tuple[bytes, bytes, bytes]:
        """(commitment48, proof48, versioned_hash32) of one blob; raises what `blob_to_commitment` raises."""
        blob = _buf(blob)
        if len(blob) != BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        coms, proofs, hashes, status = self.blob_sidecar_batch(blob, 1)
        if status[0]:
            raise error_from_status(status[0])
        return coms, proofs, hashes

    def compute_cells(self, blob: bytes) -> List[bytes]:
        """`compute_cells` (EIP-7594): the 128 cells of one blob, 2,048 bytes each; raises what `blob_to_commitment` raises."""
        blob = _buf(blob)
        if len(blob) != BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        out, status = self.compute_cells_batch(blob, 1)
        if status[0]:
            raise error_from_status(status[0])
        return [out[BYTES_PER_CELL * c:BYTES_PER_CELL * (c + 1)] for c in range(CELLS_PER_EXT_BLOB)]

    @staticmethod
    def _cell_set(cell_indices: Sequence[int], cells: Sequence[bytes]):
        """(flat cell set, mask) of one item from the spec's (indices, cells), after the spec's assertions (ValueError)"""
        cell_indices = [int(c) for c in cell_indices]
        cells = [_buf(c) for c in cells]
        if len(cell_indices) != len(cells):
            raise ValueError("recover_cells: %d indices for %d cells" % (len(cell_indices), len(cells)))
        if not CELLS_PER_EXT_BLOB // 2 <= len(cell_indices) <= CELLS_PER_EXT_BLOB:
            raise ValueError("recover_cells: %d cells, need 64..128" % len(cell_indices))
        if any(not 0 <= c < CELLS_PER_EXT_BLOB for c in cell_indices):
            raise ValueError("recover_cells: cell index out of range")
        if any(a >= b for a, b in zip(cell_indices, cell_indices[1:])):
            raise ValueError("recover_cells: cell indices must be strictly ascending")
        if any(len(c) != BYTES_PER_CELL for c in cells):
            raise ValueError("recover_cells: a cell is %d bytes" % BYTES_PER_CELL)
        flat, mask = bytearray(CELLS_PER_EXT_BLOB * BYTES_PER_CELL), bytearray(16)
        for c, cell in zip(cell_indices, cells):
            flat[BYTES_PER_CELL * c:BYTES_PER_CELL * (c + 1)] = cell
            mask[c >> 3] |= 1 << (c & 7)
        return bytes(flat), bytes(mask)

    def recover_cells(self, cell_indices: Sequence[int], cells: Sequence[bytes]) -> List[bytes]:
        """The cells half of `recover_cells_and_kzg_proofs` (EIP-7594): all 128 cells from at least 64 of them.  As the spec asserts:
        one cell per index, 64..128 of them, every index < 128, indices strictly ascending, every cell 2,048 bytes (ValueError).
        Raises BlobError InvalidFieldElement for an element >= r and, beyond the spec, CellsError Inconsistent when the cells do not lie
        on one polynomial of degree < 4096."""
        flat, mask = self._cell_set(cell_indices, cells)
        out, status = self.recover_cells_batch(flat, mask, 1)
        if status[0]:
            raise error_from_status(status[0])
        return [out[BYTES_PER_CELL * c:BYTES_PER_CELL * (c + 1)] for c in range(CELLS_PER_EXT_BLOB)]

    def compute_cells_and_proofs(self, blob: bytes):
        """`compute_cells_and_kzg_proofs` (EIP-7594): (the 128 cells of one blob, their 128 proofs of 48 bytes); raises what
        `compute_cells` raises."""
        blob = _buf(blob)
        if len(blob) != BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        cells, proofs, status = self.compute_cells_and_proofs_batch(blob, 1)
        if status[0]:
            raise error_from_status(status[0])
        return ([cells[BYTES_PER_CELL * c:BYTES_PER_CELL * (c + 1)] for c in range(CELLS_PER_EXT_BLOB)],
                [proofs[48 * c:48 * (c + 1)] for c in range(CELLS_PER_EXT_BLOB)])

    def recover_cells_and_proofs(self, cell_indices: Sequence[int], cells: Sequence[bytes]):
        """`recover_cells_and_kzg_proofs` (EIP-7594): (all 128 cells, their 128 proofs) from at least 64 cells; arguments and errors as
        `recover_cells`."""
        flat, mask = self._cell_set(cell_indices, cells)
        out, proofs, status = self.recover_cells_and_proofs_batch(flat, mask, 1)
        if status[0]:
            raise error_from_status(status[0])
        return ([out[BYTES_PER_CELL * c:BYTES_PER_CELL * (c + 1)] for c in range(CELLS_PER_EXT_BLOB)],
                [proofs[48 * c:48 * (c + 1)] for c in range(CELLS_PER_EXT_BLOB)])

    def compute_cell_proofs(self, blob: bytes, cell_indices: Sequence[int]) -> List[bytes]:
        """The proofs of the cells `cell_indices` of one blob (each what `compute_cells_and_proofs` returns for that cell), in the order
        given, at one MSM per distinct cell; raises what `compute_cells` raises, ValueError for an index out of range."""
        blob = _buf(blob)
        if len(blob) != BYTES_PER_BLOB:
            raise BlobError("InvalidLen")
        cell_indices = [int(c) for c in cell_indices]
        if any(not 0 <= c < CELLS_PER_EXT_BLOB for c in cell_indices):
            raise ValueError("compute_cell_proofs: cell index out of range")
        mask = bytearray(16)
        for c in cell_indices:
            mask[c >> 3] |= 1 << (c & 7)
        _, proofs, status = self.compute_cells_and_proofs_select_batch(blob, bytes(mask), want_cells=False)
        if status[0]:
            raise error_from_status(status[0])
        return [proofs[48 * c:48 * (c + 1)] for c in cell_indices]

    def recover_cells_and_missing_proofs(self, cell_indices: Sequence[int], cells: Sequence[bytes], proofs: Sequence[bytes]):
        """`recover_cells_and_proofs` for a node that received the cells WITH their proofs: (all 128 cells, all 128 proofs), the given
        proofs kept as they came and only the absent cells' computed.  Arguments and errors as `recover_cells`; one 48-byte proof per cell."""
        flat, mask = self._cell_set(cell_indices, cells)
        proofs = [_buf(p) for p in proofs]
        if len(proofs) != len(cells) or any(len(p) != 48 for p in proofs):
            raise ValueError("recover_cells_and_missing_proofs: one 48-byte proof per cell")
        held = bytearray(CELLS_PER_EXT_BLOB * 48)
        for c, p in zip(cell_indices, proofs):
            held[48 * int(c):48 * (int(c) + 1)] = p
        want = bytes(b ^ 0xFF for b in mask)
        out, all_proofs, status = self.recover_cells_and_proofs_select_batch(flat, mask, want, bytes(held))
        if status[0]:
            raise error_from_status(status[0])
        return ([out[BYTES_PER_CELL * c:BYTES_PER_CELL * (c + 1)] for c in range(CELLS_PER_EXT_BLOB)],
                [all_proofs[48 * c:48 * (c + 1)] for c in range(CELLS_PER_EXT_BLOB)])

    def blob_proof(self, blob: bytes, commitment: bytes) -> bytes:
        """`Setup::blob_proof` + `compress` (kzg::Error on bad input)."""
        blob, commitment = _buf(blob), _buf(commitment)
        if len(blob) != BYTES_PER_BLOB:
            raise KzgError(BlobError("InvalidLen"))
        if len(commitment) != 48:
            raise KzgError(BlsError(ECGroupError("InvalidEncoding")))
        out, status = self.compute_blob_proof_batch(blob, commitment)
        if status[0]:
            raise _kzg_error(status[0])
        return out

    def proof(self, blob: bytes, point: bytes):
        """`Setup::proof`: (proof48, y32)."""
        blob, point = _buf(blob), _buf(point)
        if len(blob) != BYTES_PER_BLOB:
            raise KzgError(BlobError("InvalidLen"))
        if len(point) != 32:
            raise KzgError(BlsError(FiniteFieldError("InvalidEncoding")))  # src/bls.rs:131-133
        proofs, ys, status = self.compute_proof_batch(blob, point)
        if status[0]:
            raise _kzg_error(status[0])
        return proofs, ys

    def evaluate_blobs(self, blobs: bytes, points32: bytes) -> Tuple[bytes, List[int]]:
        """`Polynomial::evaluate` (src/kzg/poly.rs:10-33) for n (blob, z) pairs through the verification path's evaluation
        kernel: n * 32 big-endian bytes of evaluations and the per-item status (0, BlobError InvalidFieldElement, or
        FiniteFieldError NotInFiniteField for z)."""
        blobs, points32 = _buf(blobs), _buf(points32)
        if len(points32) % 32 or len(blobs) != (len(points32) // 32) * BYTES_PER_BLOB:
            raise KzgError(BlobError("InvalidLen"))
        n = len(points32) // 32
        out = (ctypes.c_uint8 * (32 * max(n, 1)))()
        status = (ctypes.c_int32 * max(n, 1))()
        rc = self._lib.kzg_evaluate_blobs(self._h, blobs, points32, n, out, status)
        self._check(rc, "kzg_evaluate_blobs")
        return bytes(out)[:32 * n], list(status)[:n]

    def decompress_g1_batch(self, points48) -> Tuple[List["P1"], List[int]]:
        """`P1::decompress` (the crate's `Decompress` trait on `Commitment` / `Proof`, src/bls.rs:505-531) for a list (or a
        concatenation) of 48-byte encodings: the points and the per-point status (0 or an ECGroupError code)."""
        data = b"".join(points48) if isinstance(points48, (list, tuple)) else _buf(points48)
        if len(data) % 48:
            raise KzgError(BlsError(ECGroupError("InvalidEncoding")))
        n = len(data) // 48
        out = (ctypes.c_uint8 * (96 * max(n, 1)))()
        status = (ctypes.c_int32 * max(n, 1))()
        rc = self._lib.kzg_g1_decompress_batch(self._h, data, n, out, status)
        self._check(rc, "kzg_g1_decompress_batch")
        raw = bytes(out)
        return [P1(raw[96 * i:96 * i + 96]) for i in range(n)], list(status)[:n]

    def decompress_g1(self, point48: bytes) -> "P1":
        """one point; raises the reference's error (`bls::Error::ECGroup(..)`) for a rejected encoding"""
        if len(point48) != 48:
            raise BlsError(ECGroupError("InvalidEncoding"))
        pts, st = self.decompress_g1_batch(point48)
        if st[0]:
            raise BlsError(error_from_status(st[0]))
        return pts[0]

    def verify_proof(self, proof: bytes, commitment: bytes, point: bytes, evaluation: bytes) -> bool:
        proof, commitment, point, evaluation = _buf(proof), _buf(commitment), _buf(point), _buf(evaluation)
        if len(proof) != 48 or len(commitment) != 48:
            raise KzgError(BlsError(ECGroupError("InvalidEncoding")))
        if len(point) != 32 or len(evaluation) != 32:
            raise KzgError(BlsError(FiniteFieldError("InvalidEncoding")))
        return self._verdict("kzg_verify_proof", (proof, commitment, point, evaluation))

    def verify_proof_batch(self, proofs: Sequence[bytes], commitments: Sequence[bytes], points: Sequence[bytes], evals: Sequence[bytes]) -> bool:
        """`Setup::verify_proof` for n tuples in one call (the reference's private `verify_proof_batch`, src/kzg/setup.rs:115-161).
        A length mismatch is an AssertionError like verify_blob_proof_batch's; the first rejected input wins in verify_proof's
        parse order lifted to lists: every proof, then every commitment, then every point, then every evaluation."""
        assert len(proofs) == len(commitments), "assertion `left == right` failed"
        assert len(commitments) == len(points), "assertion `left == right` failed"
        assert len(points) == len(evals), "assertion `left == right` failed"
        lists = [[_buf(v) for v in seq] for seq in (proofs, commitments, points, evals)]
        # a wrong-length item never reaches the engine (the ABI takes n items of 48 / 32 bytes): it is the first error unless an
        # item BEFORE it in the parse order is rejected, so only then is the engine asked -- about the items before it
        short = None
        for kind, (seq, width) in enumerate(zip(lists, (48, 48, 32, 32))):
            bad = [i for i, v in enumerate(seq) if len(v) != width]
            if bad:
                short = (kind, bad[0])
                break
        if short is not None:
            kind, at = short
            err = KzgError(BlsError(ECGroupError("InvalidEncoding") if kind < 2 else FiniteFieldError("InvalidEncoding")))
            # everything parsed before the short item: the kinds before `kind` whole, `kind` itself up to `at`
            pts = b"".join(lists[0] if kind > 0 else lists[0][:at]) + b"".join([] if kind == 0 else (lists[1] if kind > 1 else lists[1][:at]))
            if pts:
                _, st = self.decompress_g1_batch(pts)
                hit = [c for c in st if c]
                if hit:
                    raise _kzg_error(hit[0])
            rb = _R.to_bytes(32, "big")
            scal = ([] if kind < 2 else (lists[2] if kind > 2 else lists[2][:at])) + ([] if kind < 3 else lists[3][:at])
            if any(v >= rb for v in scal):
                raise _kzg_error(7)
            raise err
        return self.verify_proof_batch_host(b"".join(lists[0]), b"".join(lists[1]), b"".join(lists[2]), b"".join(lists[3]), len(proofs))

    def verify_proof_batch_host(self, proofs, commitments, points, evals, n: int) -> bool:
        """kzg_verify_proof_batch on n CONTIGUOUS tuples in host memory: bytes-like objects or raw host addresses (ints)"""
        return self._verdict("kzg_verify_proof_batch", self._host_args(proofs, commitments, points, evals) + [n])

    def verify_cell_proof_batch(self, commitments: Sequence[bytes], cell_indices: Sequence[int], cells: Sequence[bytes], proofs: Sequence[bytes]) -> bool:
        """`verify_cell_kzg_proof_batch` (EIP-7594) with c-kzg-4844's argument shape: one commitment per cell.  Unequal lengths, an item
        of the wrong size and an index that is no uint64 are a ValueError in the caller.  Raises CellsError CellIndex for an index >= 128
        and KzgError for a rejected commitment, cell (BlobError InvalidFieldElement) or proof -- the first rejected input in the spec's
        order of assertions lifted to lists: every index, then every commitment, then every cell, then every proof."""
        n, commitments, cell_indices, cells, proofs = self._cell_lists("verify_cell_proof_batch", commitments, cell_indices, cells, proofs)
        return self.verify_cell_proof_batch_host(b"".join(commitments), cell_indices, b"".join(cells), b"".join(proofs), n)

    def verify_cell_proof_batch_host(self, commitments, cell_indices, cells, proofs, n: int) -> bool:
        """kzg_verify_cell_proof_batch on n CONTIGUOUS tuples in host memory: bytes-like objects or raw host addresses (ints); the
        indices as a sequence of ints, a bytes-like object of n native uint64 or a raw host address"""
        idx = self._cell_index_array(cell_indices, n)
        com, cells, prf = self._host_args(commitments, cells, proofs)
        return self._verdict("kzg_verify_cell_proof_batch", (com, idx, cells, prf, n), to_error=_cell_verify_error)

    def verify_cell_proof_batch_rows(self, commitments: Sequence[bytes], commitment_indices: Sequence[int], cell_indices: Sequence[int],
                                     cells: Sequence[bytes], proofs: Sequence[bytes]) -> bool:
        """`verify_cell_kzg_proof_batch` (EIP-7594) in the row-indexed form: a block's LIST of commitments, and per cell the position of
        its commitment in that list.  The verdict and the errors are verify_cell_proof_batch's on the expanded lists; an index past the
        list raises CellsError CommitmentIndex, and EVERY listed commitment is validated, referenced or not.  Unequal lengths, an item
        of the wrong size and an index that is no uint64 are a ValueError."""
        n, commitments, commitment_indices, cell_indices, cells, proofs = self._cell_rows_lists("verify_cell_proof_batch_rows", commitments, commitment_indices,
                                                                                                cell_indices, cells, proofs)
        return self.verify_cell_proof_batch_rows_host(b"".join(commitments), len(commitments), commitment_indices, cell_indices, b"".join(cells), b"".join(proofs), n)

    @staticmethod
    def _cell_rows_lists(what, commitments, commitment_indices, cell_indices, cells, proofs):
        """the row-indexed list forms' length and size checks (ValueError) -> (n, the five lists as bytes / ints)"""
        n = len(cells)
        if not (len(commitment_indices) == n and len(cell_indices) == n and len(proofs) == n):
            raise ValueError("%s: %d commitment indices, %d cell indices, %d cells, %d proofs" % (what, len(commitment_indices), len(cell_indices), n, len(proofs)))
        commitments, cells, proofs = [_buf(v) for v in commitments], [_buf(v) for v in cells], [_buf(v) for v in proofs]
        commitment_indices, cell_indices = [int(c) for c in commitment_indices], [int(c) for c in cell_indices]
        if any(len(v) != 48 for v in commitments) or any(len(v) != 48 for v in proofs):
            raise ValueError("%s: a commitment or proof is 48 bytes" % what)
        if any(len(v) != BYTES_PER_CELL for v in cells):
            raise ValueError("%s: a cell is %d bytes" % (what, BYTES_PER_CELL))
        if any(not 0 <= c < 1 << 64 for c in commitment_indices + cell_indices):
            raise ValueError("%s: an index is a uint64" % what)
        return n, commitments, commitment_indices, cell_indices, cells, proofs

    def verify_cell_proof_batch_rows_host(self, commitments, u: int, commitment_indices, cell_indices, cells, proofs, n: int) -> bool:
        """kzg_verify_cell_proof_batch_rows on u CONTIGUOUS commitments and n contiguous (commitment index, cell index, cell, proof) in host
        memory: bytes-like objects or raw host addresses (ints); either index array as in verify_cell_proof_batch_host"""
        cidx, idx = self._cell_index_array(commitment_indices, n), self._cell_index_array(cell_indices, n)
        com, cells, prf = self._host_args(commitments, cells, proofs)
        if not isinstance(com, int) and len(com) == 0:
            com = None  # an empty list: the ABI takes a null pointer with u == 0
        return self._verdict("kzg_verify_cell_proof_batch_rows", (com, u, cidx, idx, cells, prf, n), to_error=_cell_verify_error)

    def verify_cell_proof_batch_rows_dev(self, d_commitments: int, u: int, d_commitment_indices: int, d_cell_indices: int, d_cells: int, d_proofs: int, n: int,
                                         stream: int = 0) -> bool:
        """kzg_verify_cell_proof_batch_rows_dev: device pointers (16-byte aligned) to u commitments, n + n uint64 indices, n cells, n proofs"""
        return self._verdict("kzg_verify_cell_proof_batch_rows_dev", (d_commitments, u, d_commitment_indices, d_cell_indices, d_cells, d_proofs, n), (stream,),
                             to_error=_cell_verify_error)

    def verify_data_columns(self, commitments: Sequence[bytes], columns) -> bool:
        """What a PeerDAS node holds: a block's commitments (one per blob) and column sidecars.  `columns` is a list of
        (column_index, cells, proofs), cells and proofs with one entry per commitment, in the commitments' order.  Builds the two index
        arrays and calls verify_cell_proof_batch_rows."""
        return self.verify_cell_proof_batch_rows(commitments, *self._data_column_lists("verify_data_columns", len(commitments), columns))

    @staticmethod
    def _data_column_lists(what, u, columns):
        """column sidecars -> (commitment indices, cell indices, cells, proofs), column after column, a column's rows in the commitments' order"""
        rows, cols, cells, proofs = [], [], [], []
        for column_index, col_cells, col_proofs in columns:
            if len(col_cells) != u or len(col_proofs) != u:
                raise ValueError("%s: column %d has %d cells and %d proofs for %d commitments" % (what, column_index, len(col_cells), len(col_proofs), u))
            rows += range(u)
            cols += [int(column_index)] * u
            cells += list(col_cells)
            proofs += list(col_proofs)
        return rows, cols, cells, proofs

    def _rows_verdicts(self, what: str, head, n: int, u: int, tail=()):
        """a row-indexed per-item call `what`(handle, *head, n, ok_each, status, commitment_status, &ok, *tail)
        -> (ok_each, status, commitment_status, ok)"""
        ok_each, status, ok = ctypes.create_string_buffer(max(n, 1)), (ctypes.c_int32 * max(n, 1))(), ctypes.c_int32(0)
        com_status = (ctypes.c_int32 * max(u, 1))()
        rc = getattr(self._lib, what)(self._h, *head, n, ctypes.cast(ok_each, _u8p), status, com_status, ctypes.byref(ok), *tail)
        self._check(rc, what)
        if rc > 0:  # the ABI reports rejected items and commitments in its arrays, never as the call's code
            raise EngineError("%s returned %d" % (what, rc))
        return [bool(b) for b in ok_each.raw[:n]], list(status[:n]), list(com_status[:u]), bool(ok.value)

    def verify_cell_proof_batch_rows_each(self, commitments: Sequence[bytes], commitment_indices: Sequence[int], cell_indices: Sequence[int],
                                          cells: Sequence[bytes], proofs: Sequence[bytes]) -> List[Union[bool, CellsError, KzgError]]:
        """verify_cell_proof_batch_rows with one verdict per cell: True / False, or IN PLACE the error the per-cell call raises for that
        cell's expanded tuple alone -- CellsError CommitmentIndex / CellIndex, or KzgError for its commitment, cell or proof.  A listed
        commitment touches only the cells that reference it (verify_cell_proof_batch_rows_each_host also returns the list's own
        statuses).  Length and size checks are a ValueError, exactly as in verify_cell_proof_batch_rows."""
        n, commitments, commitment_indices, cell_indices, cells, proofs = self._cell_rows_lists("verify_cell_proof_batch_rows_each", commitments,
                                                                                                commitment_indices, cell_indices, cells, proofs)
        ok_each, status, _, _ = self.verify_cell_proof_batch_rows_each_host(b"".join(commitments), len(commitments), commitment_indices, cell_indices,
                                                                            b"".join(cells), b"".join(proofs), n)
        return [_cell_verify_error(status[i]) if status[i] else ok_each[i] for i in range(n)]

    def verify_cell_proof_batch_rows_each_host(self, commitments, u: int, commitment_indices, cell_indices, cells, proofs, n: int):
        """kzg_verify_cell_proof_batch_rows_each on host memory (arguments as verify_cell_proof_batch_rows_host)
        -> (ok_each: List[bool], status: List[int], commitment_status: List[int], ok: bool)"""
        cidx, idx = self._cell_index_array(commitment_indices, n), self._cell_index_array(cell_indices, n)
        com, cells, prf = self._host_args(commitments, cells, proofs)
        if not isinstance(com, int) and len(com) == 0:
            com = None  # an empty list: the ABI takes a null pointer with u == 0
        return self._rows_verdicts("kzg_verify_cell_proof_batch_rows_each", (com, u, cidx, idx, cells, prf), n, u)

    def verify_cell_proof_batch_rows_each_dev(self, d_commitments: int, u: int, d_commitment_indices: int, d_cell_indices: int, d_cells: int, d_proofs: int,
                                              n: int, stream: int = 0):
        """kzg_verify_cell_proof_batch_rows_each_dev: device pointers as verify_cell_proof_batch_rows_dev
        -> (ok_each, status, commitment_status, ok); synchronous, results in host memory"""
        return self._rows_verdicts("kzg_verify_cell_proof_batch_rows_each_dev", (d_commitments, u, d_commitment_indices, d_cell_indices, d_cells, d_proofs), n, u,
                                   (stream,))

    def verify_data_columns_each(self, commitments: Sequence[bytes], columns) -> List[list]:
        """verify_data_columns with the bad cells named: one list per column, in the given order, of the per-row results of
        verify_cell_proof_batch_rows_each (True / False / the error in place) -- which sidecar, and which cell of it, to drop."""
        u, columns = len(commitments), list(columns)
        res = self.verify_cell_proof_batch_rows_each(commitments, *self._data_column_lists("verify_data_columns_each", u, columns))
        return [res[u * k: u * (k + 1)] for k in range(len(columns))]

    def cell_row_weights(self, r: int, commitment_indices: Sequence[int], u: int, first_index: int = 0) -> List[int]:
        """w_c = sum over the items k with commitment_indices[k] == c of r^(first_index + k) mod the group order, c < u, through the kernel
        behind the row-indexed form's commitment scalars (kzg_cell_row_weights).  r >= the modulus raises KzgError, an index >= u
        CellsError CommitmentIndex."""
        n = len(commitment_indices)
        if not 0 <= r < 1 << 256 or any(not 0 <= int(c) < 1 << 64 for c in commitment_indices) or not 0 <= first_index < 1 << 64:
            raise ValueError("cell_row_weights: r is 32 bytes, indices are uint64")
        out = (ctypes.c_uint8 * (32 * max(u, 1)))()
        rc = self._lib.kzg_cell_row_weights(self._h, int(r).to_bytes(32, "big"), first_index, self._cell_index_array(commitment_indices, n), n, u, ctypes.cast(out, _u8p))
        self._check(rc, "kzg_cell_row_weights")
        if rc > 0:
            raise _cell_verify_error(rc)
        res = bytes(out)
        return [int.from_bytes(res[32 * k:32 * k + 32], "big") for k in range(u)]

    # -- the blob form (transaction-pool form): a blob's 128 cell proofs against the blob itself --------------------------------------
    @staticmethod
    def _blob_cell_lists(blobs, commitments, cell_proofs):
        """the length checks of the blob form's list calls, as verify_blob_proof_batch raises them -> (n, blobs, commitments, proofs) joined"""
        assert len(blobs) == len(commitments), "assertion `left == right` failed"
        assert len(cell_proofs) == CELLS_PER_EXT_BLOB * len(blobs), "assertion `left == right` failed"
        blobs, commitments, cell_proofs = [_buf(v) for v in blobs], [_buf(v) for v in commitments], [_buf(v) for v in cell_proofs]
        if any(len(b) != BYTES_PER_BLOB for b in blobs):
            raise KzgError(BlobError("InvalidLen"))
        if any(len(c) != 48 for c in commitments + cell_proofs):
            raise KzgError(BlsError(ECGroupError("InvalidEncoding")))
        return len(blobs), b"".join(blobs), b"".join(commitments), b"".join(cell_proofs)

    def verify_blob_cell_proofs(self, blobs: Sequence[bytes], commitments: Sequence[bytes], cell_proofs: Sequence[bytes]) -> bool:
        """Every blob's 128 cell proofs (cell_proofs[128 b + k] = proof k of blob b) against the blob and its commitment: what a
        transaction pool checks for a blob transaction of wrapper version 1 (go-ethereum's kzg4844.VerifyCellProofs).  The boolean of
        verify_cell_proof_batch_rows on the blobs' computed cells, without the cells or any index crossing to the device.  Raises as
        verify_blob_proof_batch does: AssertionError for mismatched list lengths (len(cell_proofs) == 128 len(blobs) among them),
        KzgError for a wrong-length or rejected blob, commitment or proof (every blob before any commitment, those before any proof)."""
        n, blobs, commitments, cell_proofs = self._blob_cell_lists(blobs, commitments, cell_proofs)
        return self.verify_blob_cell_proofs_batch_host(blobs, commitments, cell_proofs, n)

    def verify_blob_cell_proofs_each(self, blobs: Sequence[bytes], commitments: Sequence[bytes], cell_proofs: Sequence[bytes]) -> List[Union[bool, Exception]]:
        """verify_blob_cell_proofs with one entry per BLOB: True / False, or IN PLACE the KzgError of the blob's own first rejected input
        (blob, commitment, lowest proof) -- which transaction to drop.  A rejected blob does not touch its neighbours' verdicts."""
        n, blobs, commitments, cell_proofs = self._blob_cell_lists(blobs, commitments, cell_proofs)
        ok_each, status, _ = self.verify_blob_cell_proofs_batch_each_host(blobs, commitments, cell_proofs, n)
        return [_kzg_error(status[b]) if status[b] else ok_each[b] for b in range(n)]

    def verify_blob_cell_proofs_batch_host(self, blobs, commitments, cell_proofs, n: int) -> bool:
        """kzg_verify_blob_cell_proofs_batch on n CONTIGUOUS blobs, n commitments and 128 n cell proofs in host memory (bytes-like objects
        or raw host addresses)"""
        return self._verdict("kzg_verify_blob_cell_proofs_batch", self._host_args(blobs, commitments, cell_proofs) + [n])

    def verify_blob_cell_proofs_batch_dev(self, d_blobs: int, d_commitments: int, d_cell_proofs: int, n: int, stream: int = 0) -> bool:
        """kzg_verify_blob_cell_proofs_batch_dev: device pointers (16-byte aligned) to n blobs, n commitments, 128 n cell proofs"""
        return self._verdict("kzg_verify_blob_cell_proofs_batch_dev", (d_blobs, d_commitments, d_cell_proofs, n), (stream,))

    def verify_blob_cell_proofs_batch_each_host(self, blobs, commitments, cell_proofs, n: int):
        """kzg_verify_blob_cell_proofs_batch_each on host memory -> (ok_each, status, ok), one entry per BLOB"""
        return self._verdicts("kzg_verify_blob_cell_proofs_batch_each", self._host_args(blobs, commitments, cell_proofs), n)

    def verify_blob_cell_proofs_batch_each_dev(self, d_blobs: int, d_commitments: int, d_cell_proofs: int, n: int, stream: int = 0):
        """-> (ok_each: List[bool], status: List[int], ok: bool), one entry per BLOB; synchronous, results in host memory"""
        return self._verdicts("kzg_verify_blob_cell_proofs_batch_each_dev", (d_blobs, d_commitments, d_cell_proofs), n, (stream,))

    def blob_cell_weights(self, r: int, n_blobs: int, first_index: int = 0) -> List[int]:
        """w_b = sum_{k<128} r^(first_index + 128 b + k) mod the group order, b < n_blobs, through the kernel behind the blob form's
        commitment scalars (kzg_blob_cell_weights): cell_row_weights' values for the indices i >> 7.  r >= the modulus raises KzgError."""
        if not 0 <= r < 1 << 256 or not 0 <= first_index < 1 << 64 or n_blobs < 0:
            raise ValueError("blob_cell_weights: r is 32 bytes, first_index a uint64")
        out = (ctypes.c_uint8 * (32 * max(n_blobs, 1)))()
        rc = self._lib.kzg_blob_cell_weights(self._h, int(r).to_bytes(32, "big"), first_index, n_blobs, ctypes.cast(out, _u8p))
        self._check(rc, "kzg_blob_cell_weights")
        if rc > 0:
            raise _kzg_error(rc)
        res = bytes(out)
        return [int.from_bytes(res[32 * k:32 * k + 32], "big") for k in range(n_blobs)]

    def g1_monomial(self, first: int = 0, count: int = 64) -> List[bytes]:
        """the 48-byte encodings of the monomial G1 setup points [tau^j]_1, first <= j < first + count <= 64, which the context derives
        on first use (kzg_ctx_g1_monomial)"""
        out = (ctypes.c_uint8 * (48 * count))()
        rc = self._lib.kzg_ctx_g1_monomial(self._h, first, count, ctypes.cast(out, _u8p))
        self._check(rc, "kzg_ctx_g1_monomial")
        raw = bytes(out)
        return [raw[48 * k:48 * k + 48] for k in range(count)]

    def verify_blob_proof(self, blob: bytes, commitment: bytes, proof: bytes) -> bool:
        blob, commitment, proof = _buf(blob), _buf(commitment), _buf(proof)
        if len(blob) != BYTES_PER_BLOB:
            raise KzgError(BlobError("InvalidLen"))
        if len(commitment) != 48 or len(proof) != 48:
            raise KzgError(BlsError(ECGroupError("InvalidEncoding")))
        return self._verdict("kzg_verify_blob_proof", (blob, commitment, proof))

    def verify_blob_proof_batch(self, blobs: Sequence[bytes], commitments: Sequence[bytes], proofs: Sequence[bytes]) -> bool:
        """`Setup::verify_blob_proof_batch`.  Length mismatch panics in the
        reference (src/kzg/setup.rs:256-257) -> AssertionError here."""
        assert len(blobs) == len(commitments), "assertion `left == right` failed"
        assert len(commitments) == len(proofs), "assertion `left == right` failed"
        n = len(blobs)
        # first-error-wins order of the reference: blobs (in index order: `collect` stops at the FIRST blob that fails, whatever its
        # error -- src/kzg/setup.rs:259-262), then commitments, then proofs.  A short blob never reaches the engine (the ABI takes n
        # blobs of 131,072 bytes), so the blobs BEFORE it are checked here the way Blob::from_slice checks them (src/blob.rs:26-37):
        # (blob 0 non-canonical, blob 1 short) is InvalidFieldElement, not InvalidLen
        for i, b in enumerate(blobs):
            if len(b) != BYTES_PER_BLOB:
                if any(_has_noncanonical_element(_buf(e)) for e in blobs[:i]):
                    raise KzgError(BlobError("InvalidFieldElement"))
                raise KzgError(BlobError("InvalidLen"))
        for c in list(commitments) + list(proofs):
            if len(c) != 48:
                raise KzgError(BlsError(ECGroupError("InvalidEncoding")))
        return self._verdict("kzg_verify_blob_proof_batch", [b"".join(_buf(v) for v in seq) for seq in (blobs, commitments, proofs)] + [n])

    # -- per-item verdicts: what a loop over verify_blob_proof / verify_proof would return or raise, from one batch call ---
    def verify_blob_proof_batch_each_host(self, blobs, commitments, proofs, n: int):
        """kzg_verify_blob_proof_batch_each on n CONTIGUOUS items in host memory -> (ok_each, status, ok)"""
        return self._verdicts("kzg_verify_blob_proof_batch_each", self._host_args(blobs, commitments, proofs), n)

    def verify_proof_batch_each_host(self, proofs, commitments, points, evals, n: int):
        """kzg_verify_proof_batch_each on n CONTIGUOUS tuples in host memory -> (ok_each, status, ok)"""
        return self._verdicts("kzg_verify_proof_batch_each", self._host_args(proofs, commitments, points, evals), n)

    @staticmethod
    def _each_list(n, early, ok_each, status):
        """entry i: the wrong-length item's error, else the engine's verdict for it"""
        return [early[i] if i in early else (_kzg_error(status[i]) if status[i] else ok_each[i]) for i in range(n)]

    def verify_blob_proof_batch_each(self, blobs: Sequence[bytes], commitments: Sequence[bytes], proofs: Sequence[bytes]) -> List[Union[bool, KzgError]]:
        """Entry i is what `verify_blob_proof(blobs[i], commitments[i], proofs[i])` returns -- or the KzgError it raises, RETURNED in
        the list.  A wrong-length item gets that call's length error (blob first, then commitment, then proof) and a valid
        placeholder goes to the engine in its slot.  Length mismatches between the lists are AssertionErrors, as in the batch call."""
        assert len(blobs) == len(commitments), "assertion `left == right` failed"
        assert len(commitments) == len(proofs), "assertion `left == right` failed"
        n = len(blobs)
        items = [(_buf(b), _buf(c), _buf(p)) for b, c, p in zip(blobs, commitments, proofs)]
        early = {}
        for i, (b, c, p) in enumerate(items):
            if len(b) != BYTES_PER_BLOB:
                early[i] = KzgError(BlobError("InvalidLen"))
            elif len(c) != 48 or len(p) != 48:
                early[i] = KzgError(BlsError(ECGroupError("InvalidEncoding")))
        inf48 = bytes([0xC0]) + bytes(47)
        placeholder = (bytes(BYTES_PER_BLOB), inf48, inf48)  # the zero polynomial, committed to and opened by the point at infinity
        sent = [placeholder if i in early else it for i, it in enumerate(items)]
        ok_each, status, _ = self.verify_blob_proof_batch_each_host(b"".join(s[0] for s in sent), b"".join(s[1] for s in sent), b"".join(s[2] for s in sent), n)
        return self._each_list(n, early, ok_each, status)

    def verify_proof_batch_each(self, proofs: Sequence[bytes], commitments: Sequence[bytes], points: Sequence[bytes],
                                evals: Sequence[bytes]) -> List[Union[bool, KzgError]]:
        """Entry i is what `verify_proof(proofs[i], commitments[i], points[i], evals[i])` returns -- or the KzgError it raises,
        RETURNED in the list (verify_proof's own order: point lengths before scalar lengths, then the engine's parse order)."""
        assert len(proofs) == len(commitments), "assertion `left == right` failed"
        assert len(commitments) == len(points), "assertion `left == right` failed"
        assert len(points) == len(evals), "assertion `left == right` failed"
        n = len(proofs)
        items = [tuple(_buf(v) for v in t) for t in zip(proofs, commitments, points, evals)]
        early = {}
        for i, (p, c, z, y) in enumerate(items):
            if len(p) != 48 or len(c) != 48:
                early[i] = KzgError(BlsError(ECGroupError("InvalidEncoding")))
            elif len(z) != 32 or len(y) != 32:
                early[i] = KzgError(BlsError(FiniteFieldError("InvalidEncoding")))
        inf48 = bytes([0xC0]) + bytes(47)
        placeholder = (inf48, inf48, bytes(32), bytes(32))  # the zero polynomial opened at 0
        sent = [placeholder if i in early else it for i, it in enumerate(items)]
        ok_each, status, _ = self.verify_proof_batch_each_host(*[b"".join(s[k] for s in sent) for k in range(4)], n)
        return self._each_list(n, early, ok_each, status)

    @staticmethod
    def _cell_lists(what, commitments, cell_indices, cells, proofs):
        """the length checks of the cells calls' list forms -> (n, commitments, indices, cells, proofs) as buffers and ints"""
        n = len(commitments)
        if not (len(cell_indices) == n and len(cells) == n and len(proofs) == n):
            raise ValueError("%s: %d commitments, %d indices, %d cells, %d proofs" % (what, n, len(cell_indices), len(cells), len(proofs)))
        commitments, cells, proofs = [_buf(v) for v in commitments], [_buf(v) for v in cells], [_buf(v) for v in proofs]
        cell_indices = [int(c) for c in cell_indices]
        if any(len(v) != 48 for v in commitments) or any(len(v) != 48 for v in proofs):
            raise ValueError("%s: a commitment or proof is 48 bytes" % what)
        if any(len(v) != BYTES_PER_CELL for v in cells):
            raise ValueError("%s: a cell is %d bytes" % (what, BYTES_PER_CELL))
        if any(not 0 <= c < 1 << 64 for c in cell_indices):
            raise ValueError("%s: a cell index is a uint64" % what)
        return n, commitments, cell_indices, cells, proofs

    def verify_cell_proof_batch_each(self, commitments: Sequence[bytes], cell_indices: Sequence[int], cells: Sequence[bytes],
                                     proofs: Sequence[bytes]) -> List[Union[bool, KzgError]]:
        """Entry i is what `verify_cell_proof_batch` of tuple i alone returns -- or the error it raises (CellsError CellIndex, or KzgError
        for a commitment, cell or proof), RETURNED in the list.  The length checks are verify_cell_proof_batch's: a ValueError."""
        n, commitments, cell_indices, cells, proofs = self._cell_lists("verify_cell_proof_batch_each", commitments, cell_indices, cells, proofs)
        ok_each, status, _ = self.verify_cell_proof_batch_each_host(b"".join(commitments), cell_indices, b"".join(cells), b"".join(proofs), n)
        return [_cell_verify_error(status[i]) if status[i] else ok_each[i] for i in range(n)]

    def verify_cell_proof_batch_each_host(self, commitments, cell_indices, cells, proofs, n: int):
        """kzg_verify_cell_proof_batch_each on n CONTIGUOUS tuples in host memory (arguments as verify_cell_proof_batch_host)
        -> (ok_each, status, ok)"""
        idx = self._cell_index_array(cell_indices, n)
        com, cells, prf = self._host_args(commitments, cells, proofs)
        return self._verdicts("kzg_verify_cell_proof_batch_each", (com, idx, cells, prf), n)

    def verify_cell_proof_batch_each_dev(self, d_commitments: int, d_cell_indices: int, d_cells: int, d_proofs: int, n: int, stream: int = 0):
        """-> (ok_each: List[bool], status: List[int], ok: bool); synchronous, results in host memory"""
        return self._verdicts("kzg_verify_cell_proof_batch_each_dev", (d_commitments, d_cell_indices, d_cells, d_proofs), n, (stream,))

    def g1_monomial_lincomb(self, vectors: Sequence[Sequence[int]]) -> List[bytes]:
        """sum_j s_j [tau^j]_1 for each vector of 64 scalars (ints below r) as 96 bytes x || y big-endian, all-zero = the point at
        infinity: the kernel behind the cells *_each calls' monomial term, on its own (kzg_g1_monomial_lincomb).  A scalar >= r raises
        KzgError."""
        m = len(vectors)
        if any(len(v) != 64 for v in vectors):
            raise ValueError("g1_monomial_lincomb: a vector is 64 scalars")
        raw = b"".join(int(x).to_bytes(32, "big") for v in vectors for x in v)
        out = (ctypes.c_uint8 * (96 * max(m, 1)))()
        rc = self._lib.kzg_g1_monomial_lincomb(self._h, raw, m, ctypes.cast(out, _u8p))
        self._check(rc, "kzg_g1_monomial_lincomb")
        if rc > 0:
            raise _kzg_error(rc)
        res = bytes(out)
        return [res[96 * k:96 * k + 96] for k in range(m)]

    def verify_blob_proof_batch_host(self, blobs, commitments, proofs, n: int) -> bool:
        """kzg_verify_blob_proof_batch on n CONTIGUOUS items in host memory: bytes-like objects or raw host addresses
        (ints, e.g. the data_ptr() of a pinned tensor -- pinned memory crosses PCIe at the full rate)."""
        return self._verdict("kzg_verify_blob_proof_batch", self._host_args(blobs, commitments, proofs) + [n])

    # -- device-resident entry points (raw HIP pointers, e.g. torch.Tensor.data_ptr()) ---
    def blob_to_commitment_batch_dev(self, d_blobs: int, n: int, d_out48: int, d_status: int, stream: int = 0):
        rc = self._lib.kzg_blob_to_commitment_batch_dev(self._h, d_blobs, n, d_out48, d_status, stream)
        self._check(rc, "kzg_blob_to_commitment_batch_dev")

    def compute_blob_proof_batch_dev(self, d_blobs: int, d_commitments: int, n: int, d_out48: int, d_status: int, stream: int = 0):
        rc = self._lib.kzg_compute_blob_proof_batch_dev(self._h, d_blobs, d_commitments, n, d_out48, d_status, stream)
        self._check(rc, "kzg_compute_blob_proof_batch_dev")

    def blob_sidecar_batch_dev(self, d_blobs: int, n: int, d_commitments: int, d_proofs: int, d_versioned_hashes: int, d_status: int, stream: int = 0):
        """d_versioned_hashes = 0: no hashes wanted"""
        rc = self._lib.kzg_blob_sidecar_batch_dev(self._h, d_blobs, n, d_commitments, d_proofs, d_versioned_hashes or None, d_status, stream)
        self._check(rc, "kzg_blob_sidecar_batch_dev")

    def compute_cells_batch_dev(self, d_blobs: int, n: int, d_out_cells: int, d_status: int, stream: int = 0):
        """n blobs resident on the device -> n * 128 * 2048 bytes of cells and n int32 statuses; enqueues on `stream` and returns"""
        rc = self._lib.kzg_compute_cells_batch_dev(self._h, d_blobs, n, d_out_cells, d_status, stream)
        self._check(rc, "kzg_compute_cells_batch_dev")

    def recover_cells_batch_dev(self, d_cells: int, d_present: int, n: int, d_out_cells: int, d_status: int, stream: int = 0):
        """n cell sets and n 16-byte masks resident on the device -> n * 128 * 2048 bytes of cells and n int32 statuses; enqueues on
        `stream` and returns.  `d_out_cells` must not overlap `d_cells`."""
        rc = self._lib.kzg_recover_cells_batch_dev(self._h, d_cells, d_present, n, d_out_cells, d_status, stream)
        self._check(rc, "kzg_recover_cells_batch_dev")

    def compute_cells_and_proofs_batch_dev(self, d_blobs: int, n: int, d_out_cells: int, d_out_proofs: int, d_status: int, stream: int = 0):
        """n blobs resident on the device -> n * 128 * 2048 bytes of cells (d_out_cells = 0: no cells wanted), n * 128 * 48 bytes of cell
        proofs and n int32 statuses; enqueues on `stream` and returns"""
        rc = self._lib.kzg_compute_cells_and_proofs_batch_dev(self._h, d_blobs, n, d_out_cells or None, d_out_proofs, d_status, stream)
        self._check(rc, "kzg_compute_cells_and_proofs_batch_dev")

    def recover_cells_and_proofs_batch_dev(self, d_cells: int, d_present: int, n: int, d_out_cells: int, d_out_proofs: int, d_status: int, stream: int = 0):
        """`recover_cells_batch_dev` with n * 128 * 48 bytes of cell proofs; enqueues on `stream` and returns"""
        rc = self._lib.kzg_recover_cells_and_proofs_batch_dev(self._h, d_cells, d_present, n, d_out_cells, d_out_proofs, d_status, stream)
        self._check(rc, "kzg_recover_cells_and_proofs_batch_dev")

    def verify_blob_proof_batch_dev(self, d_blobs: int, d_commitments: int, d_proofs: int, n: int, stream: int = 0) -> bool:
        return self._verdict("kzg_verify_blob_proof_batch_dev", (d_blobs, d_commitments, d_proofs, n), (stream,))

    def verify_proof_batch_dev(self, d_proofs: int, d_commitments: int, d_points: int, d_evals: int, n: int, stream: int = 0) -> bool:
        return self._verdict("kzg_verify_proof_batch_dev", (d_proofs, d_commitments, d_points, d_evals, n), (stream,))

    def verify_blob_proof_batch_each_dev(self, d_blobs: int, d_commitments: int, d_proofs: int, n: int, stream: int = 0):
        """-> (ok_each: List[bool], status: List[int], ok: bool); synchronous, results in host memory"""
        return self._verdicts("kzg_verify_blob_proof_batch_each_dev", (d_blobs, d_commitments, d_proofs), n, (stream,))

    def verify_cell_proof_batch_dev(self, d_commitments: int, d_cell_indices: int, d_cells: int, d_proofs: int, n: int, stream: int = 0) -> bool:
        """kzg_verify_cell_proof_batch_dev: device pointers (16-byte aligned) to n commitments, n uint64 indices, n cells, n proofs"""
        return self._verdict("kzg_verify_cell_proof_batch_dev", (d_commitments, d_cell_indices, d_cells, d_proofs, n), (stream,), to_error=_cell_verify_error)

    def verify_proof_batch_each_dev(self, d_proofs: int, d_commitments: int, d_points: int, d_evals: int, n: int, stream: int = 0):
        """-> (ok_each: List[bool], status: List[int], ok: bool); synchronous, results in host memory"""
        return self._verdicts("kzg_verify_proof_batch_each_dev", (d_proofs, d_commitments, d_points, d_evals), n, (stream,))

    def compute_cells_and_proofs_select_batch_dev(self, d_blobs: int, want: bytes, n: int, d_out_cells: int, d_inout_proofs: int, d_status: int, stream: int = 0):
        """Device-resident select call: `want` is n * 16 bytes of HOST memory, read before this returns; enqueues on `stream` and returns
        without synchronising.  d_out_cells may be 0 (proofs only).  Positions of d_inout_proofs nobody wants are not written."""
        want = _buf(want)
        if len(want) != n * 16:
            raise ValueError("compute_cells_and_proofs_select_batch_dev: n * 16 bytes of mask")
        rc = self._lib.kzg_compute_cells_and_proofs_select_batch_dev(self._h, d_blobs, want, n, d_out_cells or None, d_inout_proofs, d_status, stream)
        self._check(rc, "kzg_compute_cells_and_proofs_select_batch_dev")

    def recover_cells_and_proofs_select_batch_dev(self, d_cells: int, d_present: int, want: bytes, n: int, d_out_cells: int, d_inout_proofs: int, d_status: int,
                                                  stream: int = 0):
        """Device-resident select call of recovery: `want` is HOST memory as above, `d_present` device memory as in the full call."""
        want = _buf(want)
        if len(want) != n * 16:
            raise ValueError("recover_cells_and_proofs_select_batch_dev: n * 16 bytes of mask")
        rc = self._lib.kzg_recover_cells_and_proofs_select_batch_dev(self._h, d_cells, d_present, want, n, d_out_cells, d_inout_proofs, d_status, stream)
        self._check(rc, "kzg_recover_cells_and_proofs_select_batch_dev")

    def compute_data_columns_batch_dev(self, d_blobs: int, n: int, d_out_commitments: int, d_out_column_cells: int, d_out_column_proofs: int, d_status: int,
                                       stream: int = 0):
        """n blobs resident on the device -> n * 48 bytes of commitments (d_out_commitments = 0: not wanted), the column matrices of cells
        (128 * n * 2048 bytes) and proofs (128 * n * 48) and n int32 statuses; enqueues on `stream` and returns"""
        rc = self._lib.kzg_compute_data_columns_batch_dev(self._h, d_blobs, n, d_out_commitments or None, d_out_column_cells, d_out_column_proofs, d_status, stream)
        self._check(rc, "kzg_compute_data_columns_batch_dev")

    def recover_data_columns_batch_dev(self, d_column_cells: int, present: bytes, want: Optional[bytes], n: int, d_out_column_cells: int,
                                       d_inout_column_proofs: int, d_status: int, stream: int = 0):
        """Device-resident column recovery: `present` and `want` are ONE 16-byte mask each, HOST memory, read before this returns; want =
        None goes with d_inout_column_proofs = 0 (cells only).  `d_out_column_cells` must not overlap `d_column_cells`.  Enqueues on
        `stream` and returns."""
        present, want = _buf(present), (None if want is None else _buf(want))
        if len(present) != 16 or (want is not None and len(want) != 16):
            raise ValueError("recover_data_columns_batch_dev: 16-byte masks")
        rc = self._lib.kzg_recover_data_columns_batch_dev(self._h, d_column_cells, present, want, n, d_out_column_cells, d_inout_column_proofs or None, d_status,
                                                          stream)
        self._check(rc, "kzg_recover_data_columns_batch_dev")

    def cellproof_vectors(self) -> int:
        """quotient vectors this context (all members) has committed in cell-proof calls so far, 128 per item of a full call (measurement aid)"""
        return int(self._lib.kzg_ctx_cellproof_vectors(self._h))

    def verify_each_checks(self) -> int:
        """two-pairing checks the per-item verdict calls have spent on this context so far"""
        return int(self._lib.kzg_verify_each_checks(self._h))

    def sessions_created(self) -> int:
        """verification sessions this context and its members have ever constructed (a steady state creates none)"""
        return int(self._lib.kzg_ctx_sessions_created(self._h))

    # -- device-resident SHARDED calls on a group context: one entry per member, member k's buffers resident on member k's GPU ---
    def _per_member(self, values, what):
        m = self.members
        if len(values) != m:
            raise ValueError("%s: %d entries for a context of %d members" % (what, len(values), m))
        return (ctypes.c_void_p * m)(*[int(v) if v else None for v in values])

    def _streams(self, streams):
        return self._per_member(streams, "streams") if streams is not None else None

    def _counts(self, n_local):
        if len(n_local) != self.members:
            raise ValueError("n_local: %d entries for a context of %d members" % (len(n_local), self.members))
        return (ctypes.c_uint64 * len(n_local))(*n_local)

    def blob_to_commitment_batch_group_dev(self, d_blobs, n_local, d_out48, d_status, streams=None):
        """enqueues on every member and returns without synchronising (like the *_dev calls)"""
        rc = self._lib.kzg_blob_to_commitment_batch_group_dev(self._h, self._per_member(d_blobs, "d_blobs"), self._counts(n_local), self._per_member(d_out48, "d_out48"),
                                                              self._per_member(d_status, "d_status"), self._streams(streams))
        self._check(rc, "kzg_blob_to_commitment_batch_group_dev")

    def compute_blob_proof_batch_group_dev(self, d_blobs, d_commitments, n_local, d_out48, d_status, streams=None):
        rc = self._lib.kzg_compute_blob_proof_batch_group_dev(self._h, self._per_member(d_blobs, "d_blobs"), self._per_member(d_commitments, "d_commitments"),
                                                              self._counts(n_local), self._per_member(d_out48, "d_out48"), self._per_member(d_status, "d_status"),
                                                              self._streams(streams))
        self._check(rc, "kzg_compute_blob_proof_batch_group_dev")

    def verify_blob_proof_batch_group_dev(self, d_blobs, d_commitments, d_proofs, n_local, streams=None) -> bool:
        """Setup::verify_blob_proof_batch over the members' resident shares (global order = member order): the boolean, or the
        reference's first error"""
        args = (self._per_member(d_blobs, "d_blobs"), self._per_member(d_commitments, "d_commitments"), self._per_member(d_proofs, "d_proofs"), self._counts(n_local))
        return self._verdict("kzg_verify_blob_proof_batch_group_dev", args, (self._streams(streams),))

    def verify_proof_batch_group_dev(self, d_proofs, d_commitments, d_points, d_evals, n_local, streams=None) -> bool:
        """Setup::verify_proof for the tuples of the members' resident shares (global order = member order)"""
        args = (self._per_member(d_proofs, "d_proofs"), self._per_member(d_commitments, "d_commitments"), self._per_member(d_points, "d_points"),
                self._per_member(d_evals, "d_evals"), self._counts(n_local))
        return self._verdict("kzg_verify_proof_batch_group_dev", args, (self._streams(streams),))

    def verify_proof_phase1_dev(self, d_proofs: int, d_commitments: int, d_points: int, d_evals: int, n_local: int, stream: int = 0):
        """-> (session handle, 32-byte transcript root, err8): phase 1 of verify_proof_batch; the session takes verify_phase2_dev,
        verify_session_zy and verify_session_destroy like one of verify_phase1_dev"""
        root = ctypes.create_string_buffer(32)
        err = (ctypes.c_int32 * 8)()
        sess = ctypes.c_void_p()
        rc = self._lib.kzg_verify_proof_phase1_dev(self._h, d_proofs, d_commitments, d_points, d_evals, n_local, ctypes.cast(root, ctypes.c_void_p), err,
                                                   ctypes.byref(sess), stream)
        self._check(rc, "kzg_verify_proof_phase1_dev")
        return sess, root.raw, list(err)

    def verify_phase1_dev(self, d_blobs: int, d_commitments: int, d_proofs: int, n_local: int, stream: int = 0):
        """-> (session handle, 32-byte transcript root, err6)."""
        root = ctypes.create_string_buffer(32)
        err = (ctypes.c_int32 * 6)()
        sess = ctypes.c_void_p()
        rc = self._lib.kzg_verify_phase1_dev(self._h, d_blobs, d_commitments, d_proofs, n_local, ctypes.cast(root, ctypes.c_void_p), err, ctypes.byref(sess), stream)
        self._check(rc, "kzg_verify_phase1_dev")
        return sess, root.raw, list(err)

    def verify_phase2_dev(self, session, roots: bytes, first_index: int, n_total: int) -> bytes:
        out = ctypes.create_string_buffer(192)
        rc = self._lib.kzg_verify_phase2_dev(session, _buf(roots), len(roots) // 32, first_index, n_total, ctypes.cast(out, ctypes.c_void_p))
        self._check(rc, "kzg_verify_phase2_dev")
        return out.raw

    def verify_session_tree(self, session, roots: bytes, first_index: int, n_total: int):
        """builds the per-item terms and their sum trees in a phase-1 session (r seeded as verify_phase2_dev seeds it)"""
        rc = self._lib.kzg_verify_session_tree(session, _buf(roots), len(roots) // 32, first_index, n_total)
        self._check(rc, "kzg_verify_session_tree")

    def verify_session_tree_range(self, session, lo: int, hi: int) -> bytes:
        """A || B summed over the session's local items [lo, hi), 192 bytes in verify_phase2_dev's format"""
        out = ctypes.create_string_buffer(192)
        rc = self._lib.kzg_verify_session_tree_range(session, lo, hi, ctypes.cast(out, ctypes.c_void_p))
        self._check(rc, "kzg_verify_session_tree_range")
        return out.raw

    def verify_session_zy(self, session, first: int, count: int):
        """(z bytes, y bytes) of items [first, first+count) of a phase-1 session, 32 B big-endian each"""
        z = ctypes.create_string_buffer(32 * count)
        y = ctypes.create_string_buffer(32 * count)
        rc = self._lib.kzg_verify_session_zy(session, first, count, ctypes.cast(z, ctypes.c_void_p), ctypes.cast(y, ctypes.c_void_p))
        self._check(rc, "kzg_verify_session_zy")
        return z.raw, y.raw

    def verify_session_destroy(self, session):
        self._lib.kzg_verify_session_destroy(session)

    def verify_batch_finish(self, partials: bytes) -> bool:
        ok = ctypes.c_int32(0)
        rc = self._lib.kzg_verify_batch_finish(self._h, _buf(partials), len(partials) // 192, ctypes.byref(ok))
        self._check(rc, "kzg_verify_batch_finish")
        return bool(ok.value)

    def synth_blobs_dev(self, seed: int, first_index: int, n: int, d_blobs: int, stream: int = 0):
        rc = self._lib.kzg_synth_blobs_dev(self._h, seed, first_index, n, d_blobs, stream)
        self._check(rc, "kzg_synth_blobs_dev")

    def profile_begin(self):
        self._check(self._lib.kzg_profile_begin(self._h), "kzg_profile_begin")

    PROF_KINDS = 8  # KZG_PROF_KINDS

    def profile_end(self) -> dict:
        """HIP-event kernel times since profile_begin: {"msm_ms", "msm_launches", "adds_per_blob", "kinds": {name: (ms, launches)}}."""
        ms = (ctypes.c_double * self.PROF_KINDS)()
        cnt = (ctypes.c_uint64 * self.PROF_KINDS)()
        self._check(self._lib.kzg_profile_end_kinds(self._h, ms, cnt), "kzg_profile_end_kinds")
        kinds = {self._lib.kzg_profile_kind_name(k).decode(): (ms[k], cnt[k]) for k in range(self.PROF_KINDS)}
        kinds[self.msm_kernel_name] = kinds.pop(self._lib.kzg_profile_kind_name(0).decode())  # the fixed-base MSM kernel this context runs
        return {"msm_ms": ms[0], "msm_launches": cnt[0], "adds_per_blob": self._lib.kzg_ctx_adds_per_blob(self._h), "kinds": kinds}

    def selftest_field_mul(self, lanes: int, iters: int) -> int:
        bad = ctypes.c_uint64(0)
        self._check(self._lib.kzg_selftest_field_mul(self._h, lanes, iters, ctypes.byref(bad)), "kzg_selftest_field_mul")
        return bad.value

    def microbench_valu_issue(self, waves_per_simd: int = 2, iters: int = 20000):
        """(SIMD cycles per wave-instruction of v_mad_u64_u32 at `waves_per_simd`, shader clock in GHz under that load)"""
        cyc, ghz = ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.kzg_microbench_valu_issue(self._h, waves_per_simd, iters, ctypes.byref(cyc), ctypes.byref(ghz)), "kzg_microbench_valu_issue")
        return cyc.value, ghz.value

    def clock_probe_launch(self, duration_us: int):
        """eight sleeping probe waves on the context's side stream compare the shader clock with real time for `duration_us`"""
        self._check(self._lib.kzg_clock_probe_launch(self._h, duration_us), "kzg_clock_probe_launch")

    def clock_probe_read(self):
        """(mean, lowest, highest) XCD shader clock in GHz seen by the last probe"""
        a, b, c = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.kzg_clock_probe_read(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "kzg_clock_probe_read")
        return a.value, b.value, c.value

    def microbench_fp_mul(self, lanes: int, iters: int) -> float:
        ms = ctypes.c_float(0)
        rc = self._lib.kzg_microbench_fp_mul(self._h, lanes, iters, ctypes.byref(ms))
        self._check(rc, "kzg_microbench_fp_mul")
        return ms.value
