"""Python host mirror of the reference BSMR-SDDMM interface, over libbsmr_amd.so (include/bsmr.h).

Reference interface mirrored (paths relative to the reference root):
  * sparseMatrix::CSR<float>::initializeFromMatrixFile -> load_mtx        (src/Matrix.cpp:279-480)
  * Matrix<float>::makeData                            -> make_data       (src/Matrix.cpp:117-138)
  * BSMR(alpha, delta, S) + RPHM(S, bsmr)              -> Plan            (src/BSMR.cpp:16-265)
  * sddmm_gpu(M, N, K, dA, dB, rphm, dP, logger)       -> Plan.sddmm      (src/sddmmKernel.cu:2540)
  * evaluationReordering                               -> Plan.evaluate   (src/BSMR.cpp:826-994)
Beyond the reference: the gradients of the SDDMM as SpMM over the same plan (Plan.spmm,
Plan.spmm_t, Plan.sddmm_backward), the row softmax over the plan's pattern (Plan.softmax,
Plan.softmax_backward), the fused sparse attention forward and backward (Plan.attention, Plan.attention_backward; Plan.attention_heads and Plan.attention_backward_heads over batch and heads on strided
operands), and bsmr.autograd,
which wraps SDDMM, softmax and SpMM for torch.autograd and composes them into sparse attention.

Every call goes through the HIP library; there is no CPU fallback. If the shared library is
missing the import fails loudly (build it with `make -C sddmm-gpu_amd` or
`python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes as C
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# BSMR_LIB_PATH: another build of the same library (A/B timing of kernel variants only)
LIB_PATH = os.environ.get("BSMR_LIB_PATH") or os.path.join(PKG_ROOT, "lib", "libbsmr_amd.so")

F32, F16, BF16 = 0, 1, 2
CHECK_FAILED = 7  # BSMR_ERR_CHECK
NOT_PREPARED = 8  # BSMR_ERR_NOT_PREPARED: capturing stream, launch layout not built (Plan.prepare)

ARRAYS = {
    "reorderedRows": 0, "denseCols": 1, "denseColOffsets": 2, "sparseCols": 3,
    "sparseColOffsets": 4, "sparseValueOffsets": 5, "blockOffsets": 6, "blockValues": 7,
    "sparseValues": 8, "sparseRelativeRows": 9, "sparseColIndices": 10, "dispersion": 11,
    "ascending": 12,
}

_u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")


class BsmrError(RuntimeError):
    """status: the library's integer status (include/bsmr.h bsmr_status); None when the binding
    itself raised."""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


class Tuning(C.Structure):
    """bsmr_tuning: launch-layout knobs (include/bsmr.h). "auto" = -1 (diag 0)."""
    _fields_ = [("diag", C.c_uint32), ("tile_min_f32", C.c_int32),
                ("tile_min_half", C.c_int32), ("piece_max", C.c_int32),
                ("piece_weight", C.c_float), ("shard_piece_weight", C.c_float),
                ("dense_min", C.c_float), ("orig_rows", C.c_int32), ("orig_contig", C.c_int32),
                ("dense_ks", C.c_int32), ("dense_ns", C.c_int32), ("out_staged", C.c_int32),
                ("l2_range_kb", C.c_int32), ("stage_nt", C.c_int32),
                ("rb_rows", C.c_int32), ("late_b", C.c_int32), ("item_cap", C.c_float),
                ("item_sched", C.c_int32), ("out_packed", C.c_int32),
                ("cluster_filter", C.c_int32), ("pair_min_items", C.c_int32),
                ("batches", C.c_int32), ("ptile", C.c_int32), ("ptile_tpi", C.c_int32),
                ("piece_balance", C.c_int32), ("col_blocks", C.c_int32)]


# tuning field <- its debug environment variable (bsmr_tuning_from_env)
TUNING_ENV = {f: "BSMR_" + f.upper() for f, _ in Tuning._fields_}


class PlanOptions(C.Structure):
    _fields_ = [("alpha", C.c_float), ("delta", C.c_float), ("free_mem_bytes", C.c_uint64),
                ("device", C.c_int), ("cluster_batch", C.c_uint32),
                ("exact_similarity", C.c_int), ("layout", C.c_int),
                ("lds_budget_kb", C.c_uint32), ("tuning", C.POINTER(Tuning))]


LAYOUTS = {"auto": 0, "rowblock": 1, "colmajor": 2}


class PlanStats(C.Structure):
    _fields_ = [("M", C.c_uint32), ("N", C.c_uint32), ("nnz", C.c_uint32),
                ("block_size", C.c_uint32), ("num_blocks_per_row", C.c_uint32),
                ("cluster_block_dim", C.c_uint32), ("num_clusters", C.c_int32),
                ("num_row_panels", C.c_uint32), ("num_reordered_rows", C.c_uint32),
                ("num_dense_tiles", C.c_uint32), ("max_dense_tiles_per_panel", C.c_uint32),
                ("num_residual", C.c_uint32), ("num_dense_thread_blocks", C.c_uint32),
                ("num_sparse_thread_blocks", C.c_uint32),
                ("exact_similarity_evals", C.c_uint64), ("total_similarity_evals", C.c_uint64),
                ("row_reorder_ms", C.c_float), ("col_reorder_ms", C.c_float),
                ("dense_items", C.c_uint32), ("residual_items", C.c_uint32),
                ("rb_rows", C.c_uint32 * 5), ("rb_items", C.c_uint32 * 5),
                ("rb_pieces", C.c_uint32 * 5), ("rb_entries", C.c_uint32 * 5),
                ("rb_tiles", C.c_uint32 * 5), ("rb_work_items", C.c_uint32 * 5),
                ("dense_sampled_tiles", C.c_uint32), ("rb_orig_rows", C.c_uint32),
                ("ptile_items", C.c_uint32), ("cluster_filter_used", C.c_uint32),
                ("cluster_filter_ms", C.c_float), ("rb_pairs", C.c_uint32),
                ("rb_batches", C.c_uint32), ("rb_col_blocks", C.c_uint32)]

    def as_dict(self):
        d = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            d[k] = list(v) if hasattr(v, "__len__") else v
        return d


class EvalStats(C.Structure):
    _fields_ = [("num_dense_block", C.c_int32), ("average_density", C.c_float),
                ("original_num_dense_block", C.c_int32), ("original_average_density", C.c_float),
                ("num_dense_data", C.c_int32), ("num_sparse_data", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RowStage(C.Structure):
    """bsmr_row_stage: the clustering result a multi-GPU run computes once and broadcasts."""
    _fields_ = [("M", C.c_uint32), ("N", C.c_uint32), ("nnz", C.c_uint32),
                ("block_size", C.c_uint32), ("num_blocks_per_row", C.c_uint32),
                ("cluster_block_dim", C.c_uint32), ("num_zero_rows", C.c_uint32),
                ("num_reordered_rows", C.c_uint32), ("num_clusters", C.c_int32),
                ("alpha", C.c_float), ("row_reorder_ms", C.c_float),
                ("exact_similarity_evals", C.c_uint64), ("total_similarity_evals", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def to_array(self):
        """The header as bytes in a uint8 array (to ship it in a broadcast)."""
        return np.frombuffer(bytes(self), dtype=np.uint8).copy()

    @classmethod
    def from_array(cls, a):
        return cls.from_buffer_copy(np.ascontiguousarray(a, np.uint8).tobytes())


class SpmmStats(C.Structure):
    """bsmr_spmm_stats: one side's gather lists (zeros when not built)."""
    _fields_ = [("segments", C.c_uint32), ("split_dsts", C.c_uint32), ("partials", C.c_uint32),
                ("max_list", C.c_uint32), ("chunk", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


SPMM_DIRECT = 0xFFFFFFFF  # bsmr_spmm_seg.part of a segment that writes Y itself


class SoftmaxStats(C.Structure):
    """bsmr_softmax_stats: the row softmax's item list (counts zero when not built) and the
    library's constants wave_max / block_pass."""
    _fields_ = [("items", C.c_uint32), ("packed_runs", C.c_uint32), ("wave_rows", C.c_uint32),
                ("block_rows", C.c_uint32), ("max_row", C.c_uint32), ("wave_max", C.c_uint32),
                ("block_pass", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AttentionStats(C.Structure):
    """bsmr_attention_stats: the fused attention's segment lists (counts zero when not built) and
    the library's constant chunk."""
    _fields_ = [("segments", C.c_uint32), ("split_rows", C.c_uint32), ("partials", C.c_uint32),
                ("max_row", C.c_uint32), ("chunk", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AttentionBackwardStats(C.Structure):
    """bsmr_attention_backward_stats: the fused attention backward's row and column segment lists
    and plan-owned scratch (zeros when not built) and the library's constant chunks."""
    _fields_ = [(f"{side}_{k}", C.c_uint32) for side in ("row", "col")
                for k in ("segments", "split", "partials", "max", "chunk")] + \
               [("row_scratch_bytes", C.c_uint64), ("col_scratch_bytes", C.c_uint64), ("delta_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AttentionOperand(C.Structure):
    """bsmr_attention_operand: one strided operand of the heads calls. Element [b][h][r][c] lies at
    ptr + (b batch + h head + r row + c) elements of the operand's dtype."""
    _fields_ = [("ptr", C.c_void_p), ("batch", C.c_uint64), ("head", C.c_uint64), ("row", C.c_uint64)]

    @classmethod
    def of(cls, x):
        """An AttentionOperand as it is, None (an output not asked for) as None, a (ptr, batch, head,
        row) tuple, or a 3- or 4-dimensional tensor with a contiguous last dimension (anything with
        data_ptr(), stride() and dim(): (H, rows, W) or (B, H, rows, W))."""
        if x is None or isinstance(x, cls):
            return x
        if isinstance(x, (tuple, list)):
            ptr, batch, head, row = x
            return cls(ptr, batch, head, row)
        st = tuple(x.stride())
        if x.dim() == 3:
            st = (0,) + st
        if x.dim() not in (3, 4) or st[3] != 1 or min(st) < 0:
            raise ValueError("an attention operand must be (H, rows, W) or (B, H, rows, W) with a contiguous last "
                             f"dimension, got strides {tuple(x.stride())}")
        return cls(x.data_ptr(), st[0], st[1], st[2])


# bsmr_softmax_item.kind beside a packed run's lane-group width 1 .. 64
SOFTMAX_WAVE = 0x100
SOFTMAX_BLOCK = 0x200

ABI_VERSION = 13  # include/bsmr.h BSMR_ABI_VERSION

# every symbol include/bsmr.h declares (tests check the library exports all of them)
EXPORTS = [
    "bsmr_last_error", "bsmr_abi_version", "bsmr_csr_load_mtx", "bsmr_csr_load_smtx",
    "bsmr_csr_load_snap", "bsmr_csr_load", "bsmr_csr_create",
    "bsmr_csr_info", "bsmr_csr_rowptr", "bsmr_csr_colidx", "bsmr_csr_values", "bsmr_csr_free",
    "bsmr_make_data", "bsmr_tuning_default", "bsmr_tuning_from_env",
    "bsmr_plan_options_default", "bsmr_plan_create", "bsmr_plan_recolumn",
    "bsmr_plan_destroy", "bsmr_plan_get_stats", "bsmr_plan_get_array", "bsmr_plan_evaluate",
    "bsmr_sddmm", "bsmr_sddmm_batch", "bsmr_plan_shard", "bsmr_plan_shard_dtype",
    "bsmr_shard_cuts", "bsmr_plan_shard_rebalance", "bsmr_sddmm_panels",
    "bsmr_sddmm_panels_local",
    "bsmr_plan_export_rows", "bsmr_plan_import_rows",
    "bsmr_sddmm_profile", "bsmr_sddmm_cpu", "bsmr_check_one", "bsmr_check_data",
    "bsmr_plan_check", "bsmr_check_rphm_arrays", "bsmr_cost_cuts",
    "bsmr_plan_prepare", "bsmr_plan_prepare_panels", "bsmr_plan_prepared",
    "bsmr_plan_panels_prepared",
    "bsmr_spmm", "bsmr_spmm_t", "bsmr_plan_prepare_spmm", "bsmr_plan_spmm_prepared",
    "bsmr_plan_spmm_stats", "bsmr_spmm_lists",
    "bsmr_softmax", "bsmr_softmax_backward", "bsmr_plan_prepare_softmax",
    "bsmr_plan_softmax_prepared", "bsmr_plan_softmax_stats", "bsmr_softmax_items",
    "bsmr_softmax_limits",
    "bsmr_attention", "bsmr_plan_prepare_attention", "bsmr_plan_attention_prepared",
    "bsmr_plan_attention_stats", "bsmr_attention_limits",
    "bsmr_attention_backward", "bsmr_plan_prepare_attention_backward",
    "bsmr_plan_attention_backward_prepared", "bsmr_plan_attention_backward_stats",
    "bsmr_attention_backward_limits",
    "bsmr_attention_heads", "bsmr_attention_backward_heads", "bsmr_plan_prepare_attention_heads",
    "bsmr_plan_attention_heads_prepared", "bsmr_plan_prepare_attention_backward_heads",
    "bsmr_plan_attention_backward_heads_prepared", "bsmr_attention_layout_check",
]

# include/bsmr.h BSMR_ATTENTION_MAX_BATCHES, BSMR_ATTENTION_MAX_HEADS
ATTENTION_MAX_BATCHES = 65535
ATTENTION_MAX_HEADS = 65535

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    try:
        # Share torch's HIP runtime when torch is present: torch/lib/libamdhip64.so and
        # /opt/rocm's carry the same SONAME but torch asks for the unversioned name, so loading
        # ours first would put two HIP runtimes in the process.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise BsmrError(f"HIP extension not built: {LIB_PATH} is missing "
                        "(run `make -C sddmm-gpu_amd`)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.bsmr_last_error.restype = C.c_char_p
    L.bsmr_abi_version.restype = C.c_int
    if L.bsmr_abi_version() != ABI_VERSION:  # the structs below mirror include/bsmr.h
        raise BsmrError(f"{LIB_PATH}: ABI {L.bsmr_abi_version()}, binding expects {ABI_VERSION} "
                        "(rebuild with `make -C sddmm-gpu_amd`)")
    for f in ("bsmr_csr_load_mtx", "bsmr_csr_load_smtx", "bsmr_csr_load_snap", "bsmr_csr_load"):
        getattr(L, f).argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.bsmr_csr_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, C.POINTER(vp)]
    L.bsmr_csr_info.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                C.POINTER(C.c_uint32)]
    L.bsmr_csr_rowptr.restype = C.POINTER(C.c_uint32)
    L.bsmr_csr_rowptr.argtypes = [vp]
    L.bsmr_csr_colidx.restype = C.POINTER(C.c_uint32)
    L.bsmr_csr_colidx.argtypes = [vp]
    L.bsmr_csr_values.restype = C.POINTER(C.c_float)
    L.bsmr_csr_values.argtypes = [vp]
    L.bsmr_csr_free.argtypes = [vp]
    L.bsmr_make_data.argtypes = [C.c_uint64, _f32p]
    L.bsmr_plan_options_default.argtypes = [C.POINTER(PlanOptions)]
    L.bsmr_tuning_default.argtypes = [C.POINTER(Tuning)]
    L.bsmr_tuning_from_env.argtypes = [C.POINTER(Tuning)]
    L.bsmr_tuning_from_env.restype = C.c_int
    L.bsmr_plan_create.argtypes = [_u32p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.POINTER(PlanOptions), C.POINTER(vp)]
    L.bsmr_plan_recolumn.argtypes = [vp, C.c_float]
    L.bsmr_plan_destroy.argtypes = [vp]
    L.bsmr_plan_get_stats.argtypes = [vp, C.POINTER(PlanStats)]
    L.bsmr_plan_get_array.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_uint64)]
    L.bsmr_plan_evaluate.argtypes = [vp, C.POINTER(EvalStats)]
    L.bsmr_sddmm.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, vp]
    L.bsmr_sddmm_batch.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, C.c_int, vp, vp]
    L.bsmr_plan_shard.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint32)]
    L.bsmr_plan_shard_dtype.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.bsmr_shard_cuts.argtypes = [_u32p, _u32p, C.c_uint32, C.c_uint32, C.c_int, _u32p]
    L.bsmr_plan_shard_rebalance.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, _u32p, _f32p, _u32p]
    L.bsmr_cost_cuts.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp, _u32p]
    L.bsmr_sddmm_panels.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, C.c_uint32,
                                    C.c_uint32, vp]
    L.bsmr_sddmm_panels_local.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, C.c_uint32,
                                          C.c_uint32, vp]
    L.bsmr_plan_export_rows.argtypes = [vp, C.POINTER(RowStage), vp]
    L.bsmr_plan_import_rows.argtypes = [_u32p, _u32p, C.POINTER(RowStage), vp,
                                        C.POINTER(PlanOptions), C.POINTER(vp)]
    L.bsmr_sddmm_cpu.argtypes = [_u32p, _u32p, C.c_uint32, C.c_uint32, C.c_uint32, _f32p, _f32p,
                                 _f32p, C.c_int]
    L.bsmr_check_one.restype = C.c_int
    L.bsmr_check_one.argtypes = [C.c_float, C.c_float]
    L.bsmr_check_data.restype = C.c_uint64
    L.bsmr_check_data.argtypes = [C.c_uint64, _f32p, _f32p, C.c_int]
    L.bsmr_sddmm_profile.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, C.c_int, vp,
                                     C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(C.c_float)]
    for f in ("bsmr_plan_prepare", "bsmr_plan_prepared"):
        getattr(L, f).argtypes = [vp, C.c_uint32, C.c_int]
        getattr(L, f).restype = C.c_int
    for f in ("bsmr_plan_prepare_panels", "bsmr_plan_panels_prepared"):
        getattr(L, f).argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int]
        getattr(L, f).restype = C.c_int
    for f in ("bsmr_spmm", "bsmr_spmm_t"):
        getattr(L, f).argtypes = [vp, vp, vp, C.c_uint32, C.c_int, vp, vp]
        getattr(L, f).restype = C.c_int
    L.bsmr_plan_prepare_spmm.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32]
    L.bsmr_plan_prepare_spmm.restype = C.c_int
    L.bsmr_plan_spmm_prepared.argtypes = [vp, C.c_uint32, C.c_int]
    L.bsmr_plan_spmm_prepared.restype = C.c_int
    L.bsmr_plan_spmm_stats.argtypes = [vp, C.c_int, C.POINTER(SpmmStats)]
    L.bsmr_plan_spmm_stats.restype = C.c_int
    L.bsmr_spmm_lists.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p, C.c_int,
                                  C.c_uint32, vp, C.c_uint32, vp, C.POINTER(C.c_uint64), vp, vp]
    L.bsmr_spmm_lists.restype = C.c_int
    L.bsmr_softmax.argtypes = [vp, vp, C.c_float, vp, vp]
    L.bsmr_softmax.restype = C.c_int
    L.bsmr_softmax_backward.argtypes = [vp, vp, vp, C.c_float, vp, vp]
    L.bsmr_softmax_backward.restype = C.c_int
    for f in ("bsmr_plan_prepare_softmax", "bsmr_plan_softmax_prepared"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = C.c_int
    L.bsmr_plan_softmax_stats.argtypes = [vp, C.POINTER(SoftmaxStats)]
    L.bsmr_plan_softmax_stats.restype = C.c_int
    L.bsmr_softmax_items.argtypes = [C.c_uint32, vp, vp, C.POINTER(C.c_uint64)]
    L.bsmr_softmax_items.restype = C.c_int
    L.bsmr_softmax_limits.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.bsmr_softmax_limits.restype = None
    L.bsmr_attention.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_float, vp, vp, vp]
    L.bsmr_attention.restype = C.c_int
    for f in ("bsmr_plan_prepare_attention", "bsmr_plan_attention_prepared"):
        getattr(L, f).argtypes = [vp, C.c_uint32, C.c_uint32]
        getattr(L, f).restype = C.c_int
    L.bsmr_plan_attention_stats.argtypes = [vp, C.POINTER(AttentionStats)]
    L.bsmr_plan_attention_stats.restype = C.c_int
    L.bsmr_attention_limits.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.bsmr_attention_limits.restype = None
    L.bsmr_attention_backward.argtypes = [vp] * 7 + [C.c_uint32, C.c_uint32, C.c_int, C.c_float] + [vp] * 4
    L.bsmr_attention_backward.restype = C.c_int
    for f in ("bsmr_plan_prepare_attention_backward", "bsmr_plan_attention_backward_prepared"):
        getattr(L, f).argtypes = [vp, C.c_uint32, C.c_uint32]
        getattr(L, f).restype = C.c_int
    L.bsmr_plan_attention_backward_stats.argtypes = [vp, C.POINTER(AttentionBackwardStats)]
    L.bsmr_plan_attention_backward_stats.restype = C.c_int
    L.bsmr_attention_backward_limits.argtypes = [C.POINTER(C.c_uint32)] * 3
    L.bsmr_attention_backward_limits.restype = None
    op = C.POINTER(AttentionOperand)
    L.bsmr_attention_heads.argtypes = [vp, C.c_uint32, C.c_uint32, op, op, op, C.c_uint32, C.c_uint32, C.c_int,
                                       C.c_float, op, vp, vp]
    L.bsmr_attention_heads.restype = C.c_int
    L.bsmr_attention_backward_heads.argtypes = [vp, C.c_uint32, C.c_uint32, op, op, op, op, op, vp, C.c_uint32,
                                                C.c_uint32, C.c_int, C.c_float, op, op, op, vp]
    L.bsmr_attention_backward_heads.restype = C.c_int
    for f in ("bsmr_plan_prepare_attention_heads", "bsmr_plan_attention_heads_prepared",
              "bsmr_plan_prepare_attention_backward_heads", "bsmr_plan_attention_backward_heads_prepared"):
        getattr(L, f).argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32]
        getattr(L, f).restype = C.c_int
    L.bsmr_attention_layout_check.argtypes = [op] + [C.c_uint32] * 5 + [C.c_int]
    L.bsmr_attention_layout_check.restype = C.c_int
    L.bsmr_plan_check.argtypes = [vp, C.c_uint32, C.c_int, C.c_int]
    L.bsmr_plan_check.restype = C.c_int
    L.bsmr_check_rphm_arrays.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32] + [_u32p] * 2 + \
        [C.c_uint32] + [_u32p] * 11 + [C.c_float, C.c_int]
    L.bsmr_check_rphm_arrays.restype = C.c_int
    _lib = L
    return L


def _check(status, what):
    if status != 0:
        msg = lib().bsmr_last_error().decode(errors="replace")
        raise BsmrError(f"{what} failed with status {status}: {msg}", status)


_default_tuning = {}


def tuning_from_env(env=None):
    """The tuning knobs given as BSMR_<FIELD> variables, as a {field: value} dict for Plan(tuning=).
    env: a mapping (e.g. a test's parameters); None reads this process's environment through the
    library's own parser (bsmr_tuning_from_env). The library never reads them by itself."""
    t = Tuning()
    lib().bsmr_tuning_default(C.byref(t))
    base = {f: getattr(t, f) for f, _ in Tuning._fields_}
    if env is None:
        lib().bsmr_tuning_from_env(C.byref(t))
        return {f: getattr(t, f) for f, _ in Tuning._fields_ if getattr(t, f) != base[f]}
    out = {}
    for f, _ in Tuning._fields_:
        v = env.get(TUNING_ENV[f])
        if v is None:
            continue
        if f in ("orig_rows", "out_staged", "stage_nt", "item_sched", "out_packed", "cluster_filter",
                 "batches", "ptile", "piece_balance"):  # tri-state: "0" never, "1" always, else auto
            out[f] = 0 if v.startswith("0") else 1 if v.startswith("1") else -1
        elif f in ("piece_weight", "shard_piece_weight", "dense_min", "item_cap"):
            out[f] = float(v)
        else:
            out[f] = int(v)
    return out


def set_default_tuning(tuning):
    """Tuning applied to every later Plan built without an explicit `tuning` (tools and bench
    call this with tuning_from_env() so their A/B runs can be steered from the environment)."""
    global _default_tuning
    _default_tuning = dict(tuning or {})


def _tuning_struct(tuning):
    t = Tuning()
    lib().bsmr_tuning_default(C.byref(t))
    for k, v in (tuning or {}).items():
        if k not in TUNING_ENV:
            raise BsmrError(f"unknown tuning field {k!r}")
        setattr(t, k, v)
    return t


def make_data(n):
    """Matrix<float>::makeData stream: default-seeded mt19937, uniform [0, 2)."""
    out = np.empty(int(n), np.float32)
    lib().bsmr_make_data(out.size, out)
    return out


class Csr:
    """Host CSR (uint32 rowptr/colidx), as sparseMatrix::CSR<float>."""

    def __init__(self, handle):
        self.h = handle
        M, N, nnz = C.c_uint32(), C.c_uint32(), C.c_uint32()
        lib().bsmr_csr_info(handle, C.byref(M), C.byref(N), C.byref(nnz))
        self.M, self.N, self.nnz = M.value, N.value, nnz.value

    @classmethod
    def load_mtx(cls, path, verbose=False):
        return cls._load("bsmr_csr_load_mtx", path, verbose)

    @classmethod
    def load(cls, path, verbose=False):
        """Any supported file (.mtx/.mmio, .smtx, SNAP .txt) by suffix; None if rejected."""
        return cls._load("bsmr_csr_load", path, verbose)

    @classmethod
    def _load(cls, fn, path, verbose):
        h = C.c_void_p()
        st = getattr(lib(), fn)(path.encode(), 1 if verbose else 0, C.byref(h))
        if st != 0:
            return None
        return cls(h)

    @classmethod
    def from_arrays(cls, M, N, rowptr, colidx):
        rowptr = np.ascontiguousarray(rowptr, np.uint32)
        colidx = np.ascontiguousarray(colidx, np.uint32)
        h = C.c_void_p()
        _check(lib().bsmr_csr_create(M, N, len(colidx), rowptr, colidx, C.byref(h)),
               "bsmr_csr_create")
        return cls(h)

    @property
    def rowptr(self):
        return np.ctypeslib.as_array(lib().bsmr_csr_rowptr(self.h), shape=(self.M + 1,)).copy()

    @property
    def colidx(self):
        return np.ctypeslib.as_array(lib().bsmr_csr_colidx(self.h), shape=(self.nnz,)).copy()

    @property
    def values(self):
        return np.ctypeslib.as_array(lib().bsmr_csr_values(self.h), shape=(self.nnz,)).copy()

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.bsmr_csr_free(self.h)
            self.h = None


def load_mtx(path, verbose=False):
    return Csr.load_mtx(path, verbose)


def load(path, verbose=False):
    return Csr.load(path, verbose)


class Plan:
    """Device-resident BSMR plan (reordered rows, dense 16x16 tiles, residual lists)."""

    def __init__(self, M, N, rowptr, colidx, alpha=0.3, delta=0.3, free_mem_bytes=0, device=0,
                 cluster_batch=0, exact_similarity=False, layout="auto", lds_budget_kb=0,
                 tuning=None, _row_stage=None):
        """tuning: {bsmr_tuning field: value} (None = the process default, normally empty)."""
        rowptr = np.ascontiguousarray(rowptr, np.uint32)
        colidx = np.ascontiguousarray(colidx, np.uint32)
        o = PlanOptions()
        lib().bsmr_plan_options_default(C.byref(o))
        o.alpha = float(np.float32(alpha))
        o.delta = float(np.float32(delta))
        o.free_mem_bytes = int(free_mem_bytes)
        o.device = int(device)
        o.cluster_batch = int(cluster_batch)
        o.exact_similarity = 1 if exact_similarity else 0
        o.layout = LAYOUTS[layout]
        o.lds_budget_kb = int(lds_budget_kb)
        self._tuning = _tuning_struct(_default_tuning if tuning is None else tuning)
        o.tuning = C.pointer(self._tuning)
        self.M, self.N, self.nnz = int(M), int(N), int(len(colidx))
        h = C.c_void_p()
        if _row_stage is None:
            _check(lib().bsmr_plan_create(rowptr, colidx, M, N, len(colidx), C.byref(o),
                                          C.byref(h)), "bsmr_plan_create")
        else:
            hdr, rows_ptr = _row_stage
            _check(lib().bsmr_plan_import_rows(rowptr, colidx, C.byref(hdr), rows_ptr,
                                               C.byref(o), C.byref(h)), "bsmr_plan_import_rows")
        self.h = h

    @classmethod
    def from_row_stage(cls, rowptr, colidx, hdr, rows, delta=0.3, device=0, layout="auto",
                       lds_budget_kb=0, tuning=None):
        """bsmr_plan_import_rows: the plan of an exported row stage (no clustering). rows: a
        uint32 numpy array, or an int device pointer (e.g. a broadcast tensor's data_ptr())."""
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows, np.uint32)
            ptr = rows.ctypes.data
        else:
            ptr = int(rows)
        return cls(hdr.M, hdr.N, rowptr, colidx, alpha=hdr.alpha, delta=delta, device=device,
                   layout=layout, lds_budget_kb=lds_budget_kb, tuning=tuning,
                   _row_stage=(hdr, ptr))

    def export_rows(self, rows_out=None):
        """bsmr_plan_export_rows: (header, rows). rows_out: None (a numpy array is returned) or
        an int pointer (host or device) receiving num_reordered_rows uint32."""
        hdr = RowStage()
        _check(lib().bsmr_plan_export_rows(self.h, C.byref(hdr), None), "bsmr_plan_export_rows")
        if rows_out is None:
            rows = np.empty(max(hdr.num_reordered_rows, 1), np.uint32)
            _check(lib().bsmr_plan_export_rows(self.h, C.byref(hdr), rows.ctypes.data),
                   "bsmr_plan_export_rows")
            return hdr, rows[:hdr.num_reordered_rows]
        _check(lib().bsmr_plan_export_rows(self.h, C.byref(hdr), int(rows_out)),
               "bsmr_plan_export_rows")
        return hdr, None

    def recolumn(self, delta):
        _check(lib().bsmr_plan_recolumn(self.h, float(np.float32(delta))), "bsmr_plan_recolumn")

    def stats(self):
        s = PlanStats()
        _check(lib().bsmr_plan_get_stats(self.h, C.byref(s)), "bsmr_plan_get_stats")
        return s.as_dict()

    def array(self, name):
        which = ARRAYS[name]
        n = C.c_uint64()
        _check(lib().bsmr_plan_get_array(self.h, which, None, C.byref(n)), "bsmr_plan_get_array")
        out = np.empty(n.value, np.uint32)
        if n.value:
            _check(lib().bsmr_plan_get_array(self.h, which, out.ctypes.data, C.byref(n)),
                   "bsmr_plan_get_array")
        return out

    def evaluate(self):
        e = EvalStats()
        _check(lib().bsmr_plan_evaluate(self.h, C.byref(e)), "bsmr_plan_evaluate")
        return e.as_dict()

    def check(self, K=0, dtype=F32, verbose=True):
        """bsmr_plan_check (the reference's check_rphm, BSMR.cpp:932-953): (True, "") when the plan
        and, for K > 0, the launch layout of (K, dtype) pass; (False, first error) otherwise."""
        st = lib().bsmr_plan_check(self.h, K, dtype, 1 if verbose else 0)
        if st == 0:
            return True, ""
        msg = lib().bsmr_last_error().decode(errors="replace")
        if st != CHECK_FAILED:
            raise BsmrError(f"bsmr_plan_check failed with status {st}: {msg}")
        return False, msg

    def prepare(self, K, dtype=F32, panels=None, local=False):
        """Build now what the first sddmm / sddmm_batch of (K, dtype) would build inside the call
        (bsmr_plan_prepare); panels=(p0, p1): the same for sddmm_panels over that range, or with
        local=True for sddmm_panels_local (bsmr_plan_prepare_panels). Synchronous; afterwards the
        launch touches no host state and can be captured into a HIP graph. recolumn() drops what
        this built."""
        if panels is None:
            _check(lib().bsmr_plan_prepare(self.h, K, dtype), "bsmr_plan_prepare")
        else:
            _check(lib().bsmr_plan_prepare_panels(self.h, K, dtype, panels[0], panels[1],
                                                  1 if local else 0), "bsmr_plan_prepare_panels")

    def prepared(self, K, dtype=F32, panels=None, local=False):
        """Whether the matching launch would allocate, copy or synchronise nothing
        (bsmr_plan_prepared / bsmr_plan_panels_prepared; no device call)."""
        if panels is None:
            return bool(lib().bsmr_plan_prepared(self.h, K, dtype))
        return bool(lib().bsmr_plan_panels_prepared(self.h, K, dtype, panels[0], panels[1],
                                                    1 if local else 0))

    def sddmm(self, dA, dB, K, dP, stream=0, dtype=F32):
        """dA, dB, dP: device pointers (int) — e.g. torch tensor .data_ptr()."""
        _check(lib().bsmr_sddmm(self.h, dA, dB, K, dtype, dP, stream or None), "bsmr_sddmm")

    def sddmm_batch(self, num_batch, dA, dB, K, dP, stream=0, dtype=F32):
        """num_batch (A, B) pairs: batch b at dA + b*M*K, dB + b*N*K elements, dP + b*nnz."""
        _check(lib().bsmr_sddmm_batch(self.h, num_batch, dA, dB, K, dtype, dP, stream or None),
               "bsmr_sddmm_batch")

    def sddmm_panels(self, dA, dB, K, dP, p0, p1, stream=0, dtype=F32):
        _check(lib().bsmr_sddmm_panels(self.h, dA, dB, K, dtype, dP, p0, p1, stream or None),
               "bsmr_sddmm_panels")

    def sddmm_panels_local(self, dA_local, dB, K, dP, p0, p1, stream=0, dtype=F32):
        """Shard launch with a shard-local A: rows of reordered positions [16 p0, 16 p1)."""
        _check(lib().bsmr_sddmm_panels_local(self.h, dA_local, dB, K, dtype, dP, p0, p1,
                                             stream or None), "bsmr_sddmm_panels_local")

    def spmm(self, dV, dB, K, dY, stream=0, dtype=F32):
        """bsmr_spmm: Y (M x K fp32) = S(V) B. dV (fp32, nnz, CSR order), dB (N x K of dtype) and
        dY are device pointers; with V = dP this is dA of sddmm. Every element of Y is written."""
        _check(lib().bsmr_spmm(self.h, dV, dB, K, dtype, dY, stream or None), "bsmr_spmm")

    def spmm_t(self, dV, dA, K, dY, stream=0, dtype=F32):
        """bsmr_spmm_t: Y (N x K fp32) = S(V)^T A; with V = dP this is dB of sddmm."""
        _check(lib().bsmr_spmm_t(self.h, dV, dA, K, dtype, dY, stream or None), "bsmr_spmm_t")

    def prepare_spmm(self, K, sides=3, chunk=0):
        """bsmr_plan_prepare_spmm: build now the gather lists and scratch of spmm (sides & 1) and
        spmm_t (sides & 2) at K, so that their first launch can be captured. chunk: entries per
        segment, 0 = what is built already, else the default."""
        _check(lib().bsmr_plan_prepare_spmm(self.h, K, sides, chunk), "bsmr_plan_prepare_spmm")

    def spmm_prepared(self, K, sides=3):
        return bool(lib().bsmr_plan_spmm_prepared(self.h, K, sides))

    def spmm_stats(self, side):
        s = SpmmStats()
        _check(lib().bsmr_plan_spmm_stats(self.h, side, C.byref(s)), "bsmr_plan_spmm_stats")
        return s.as_dict()

    def softmax(self, dP, dW, scale=1.0, stream=0):
        """bsmr_softmax: per row of S, W = softmax(scale * P) over the row's stored entries (dP,
        dW: device pointers to nnz fp32 in CSR order; dW == dP works in place). The maximum is
        subtracted before the scaling. scale: finite and > 0. -inf entries get weight 0, a row of
        nothing but -inf all zeros, a row with a NaN or +inf all NaN; empty rows write nothing."""
        _check(lib().bsmr_softmax(self.h, dP, scale, dW, stream or None), "bsmr_softmax")

    def softmax_backward(self, dW, dG, dGP, scale=1.0, stream=0):
        """bsmr_softmax_backward: dGP = scale * W * (G - sum_row W G), the gradient of
        Plan.softmax at the same scale from its result W and G = dL/dW (dGP == dG works in place)."""
        _check(lib().bsmr_softmax_backward(self.h, dW, dG, scale, dGP, stream or None),
               "bsmr_softmax_backward")

    def prepare_softmax(self):
        """bsmr_plan_prepare_softmax: build the softmax item list now, so that the first softmax
        launch can be captured."""
        _check(lib().bsmr_plan_prepare_softmax(self.h), "bsmr_plan_prepare_softmax")

    def softmax_prepared(self):
        return bool(lib().bsmr_plan_softmax_prepared(self.h))

    def softmax_stats(self):
        s = SoftmaxStats()
        _check(lib().bsmr_plan_softmax_stats(self.h, C.byref(s)), "bsmr_plan_softmax_stats")
        return s.as_dict()

    def attention(self, dQ, dK, dV, D, Dv, dO, dLse=0, scale=1.0, stream=0, dtype=F32):
        """bsmr_attention: O (M x Dv fp32) = softmax(scale * S .* (Q K^T)) V per row of S in one
        launch (two with split rows), without the nnz-sized scores and weights; dLse (M fp32, 0 =
        none) receives max * scale + ln(sum). dQ (M x D), dK (N x D), dV (N x Dv) of one dtype;
        every element of O and LSE is written."""
        _check(lib().bsmr_attention(self.h, dQ, dK, dV, D, Dv, dtype, scale, dO, dLse or None,
                                    stream or None), "bsmr_attention")

    def prepare_attention(self, D, Dv):
        """bsmr_plan_prepare_attention: build the attention lists and the scratch of the split rows
        for Dv now, so that the first attention launch can be captured."""
        _check(lib().bsmr_plan_prepare_attention(self.h, D, Dv), "bsmr_plan_prepare_attention")

    def attention_prepared(self, D, Dv):
        return bool(lib().bsmr_plan_attention_prepared(self.h, D, Dv))

    def attention_stats(self):
        s = AttentionStats()
        _check(lib().bsmr_plan_attention_stats(self.h, C.byref(s)), "bsmr_plan_attention_stats")
        return s.as_dict()

    def attention_backward(self, dQ, dK, dV, dO, dGO, dLse, D, Dv, dGQ=0, dGK=0, dGV=0, scale=1.0, stream=0,
                           dtype=F32):
        """bsmr_attention_backward: GQ (M x D), GK (N x D), GV (N x Dv) fp32, the gradients of
        Plan.attention from Q, K, V, the forward's O and LSE and GO = dL/dO (fp32), without an
        nnz-sized tensor. Any output may be 0 (skipped); not all three."""
        _check(lib().bsmr_attention_backward(self.h, dQ, dK, dV, dO, dGO, dLse, D, Dv, dtype, scale,
                                             dGQ or None, dGK or None, dGV or None, stream or None),
               "bsmr_attention_backward")

    def prepare_attention_backward(self, D, Dv):
        """bsmr_plan_prepare_attention_backward: build the backward's lists, delta and scratch for
        (D, Dv) now, so that the first attention_backward launch can be captured."""
        _check(lib().bsmr_plan_prepare_attention_backward(self.h, D, Dv), "bsmr_plan_prepare_attention_backward")

    def attention_backward_prepared(self, D, Dv):
        return bool(lib().bsmr_plan_attention_backward_prepared(self.h, D, Dv))

    def attention_backward_stats(self):
        s = AttentionBackwardStats()
        _check(lib().bsmr_plan_attention_backward_stats(self.h, C.byref(s)), "bsmr_plan_attention_backward_stats")
        return s.as_dict()

    def attention_heads(self, batches, heads, Q, K, V, D, Dv, O, dLse=0, scale=1.0, stream=0, dtype=F32):
        """bsmr_attention_heads: Plan.attention over batches x heads slices of the plan's pattern in
        one call (at most two launches). Q, K, V, O: AttentionOperand.of() of each (a tensor view, a
        (ptr, batch, head, row) tuple or an AttentionOperand; strides in elements); O fp32; dLse a
        dense (batches, heads, M) fp32 pointer or 0."""
        ops = [AttentionOperand.of(x) for x in (Q, K, V, O)]
        ref = [None if o is None else C.byref(o) for o in ops]
        _check(lib().bsmr_attention_heads(self.h, batches, heads, ref[0], ref[1], ref[2], D, Dv, dtype, scale, ref[3],
                                          dLse or None, stream or None), "bsmr_attention_heads")

    def attention_backward_heads(self, batches, heads, Q, K, V, O, GO, dLse, D, Dv, GQ=None, GK=None, GV=None, scale=1.0,
                                 stream=0, dtype=F32):
        """bsmr_attention_backward_heads: Plan.attention_backward over batches x heads slices in one
        call (at most five launches). Operands as in attention_heads; O, GO and the outputs fp32; an
        output that is None is skipped (not all three)."""
        ops = [AttentionOperand.of(x) for x in (Q, K, V, O, GO, GQ, GK, GV)]
        ref = [None if o is None else C.byref(o) for o in ops]
        _check(lib().bsmr_attention_backward_heads(self.h, batches, heads, *ref[:5], dLse or None, D, Dv, dtype, scale,
                                                   *ref[5:], stream or None), "bsmr_attention_backward_heads")

    def prepare_attention_heads(self, D, Dv, slices):
        """bsmr_plan_prepare_attention_heads: the attention lists and the scratch of `slices` slices
        at Dv now, so that the first attention_heads launch can be captured."""
        _check(lib().bsmr_plan_prepare_attention_heads(self.h, D, Dv, slices), "bsmr_plan_prepare_attention_heads")

    def attention_heads_prepared(self, D, Dv, slices):
        return bool(lib().bsmr_plan_attention_heads_prepared(self.h, D, Dv, slices))

    def prepare_attention_backward_heads(self, D, Dv, slices):
        """bsmr_plan_prepare_attention_backward_heads: the backward's lists, delta and scratch of
        `slices` slices at (D, Dv) now."""
        _check(lib().bsmr_plan_prepare_attention_backward_heads(self.h, D, Dv, slices),
               "bsmr_plan_prepare_attention_backward_heads")

    def attention_backward_heads_prepared(self, D, Dv, slices):
        return bool(lib().bsmr_plan_attention_backward_heads_prepared(self.h, D, Dv, slices))

    def sddmm_backward(self, dG, dA, dB, K, dGA, dGB, stream=0, dtype=F32):
        """The gradients of P = sddmm(A, B) from dG = dL/dP (fp32, nnz): dGA (M x K fp32) =
        S(G) B and dGB (N x K fp32) = S(G)^T A. Either output may be 0: that side is skipped."""
        if dGA:
            self.spmm(dG, dB, K, dGA, stream=stream, dtype=dtype)
        if dGB:
            self.spmm_t(dG, dA, K, dGB, stream=stream, dtype=dtype)

    def shard(self, K, rank, world, dtype=F32):
        """Panel range [p0, p1) of `rank` (bsmr_plan_shard_dtype)."""
        p0, p1 = C.c_uint32(), C.c_uint32()
        _check(lib().bsmr_plan_shard_dtype(self.h, K, dtype, rank, world, C.byref(p0),
                                           C.byref(p1)), "bsmr_plan_shard_dtype")
        return p0.value, p1.value

    def shard_rebalance(self, K, world, prev_cuts, shard_ms, dtype=F32):
        """Cuts [0 = c_0 <= ... <= c_world = P] re-balanced by measured shard times
        (bsmr_plan_shard_rebalance); prev_cuts: the cuts those times were measured on."""
        prev = np.ascontiguousarray(prev_cuts, np.uint32)
        ms = np.ascontiguousarray(shard_ms, np.float32)
        if len(prev) != world + 1 or len(ms) != world:
            raise ValueError("shard_rebalance: prev_cuts needs world + 1 entries, shard_ms world")
        cuts = np.zeros(world + 1, np.uint32)
        _check(lib().bsmr_plan_shard_rebalance(self.h, K, dtype, world, prev, ms, cuts),
               "bsmr_plan_shard_rebalance")
        return [int(c) for c in cuts]

    def profile(self, dA, dB, K, dP, iters=10, stream=0, dtype=F32):
        d, r, t = C.c_float(), C.c_float(), C.c_float()
        _check(lib().bsmr_sddmm_profile(self.h, dA, dB, K, dtype, dP, iters, stream or None,
                                        C.byref(d), C.byref(r), C.byref(t)),
               "bsmr_sddmm_profile")
        return {"dense_ms": d.value, "residual_ms": r.value, "total_ms": t.value}

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.bsmr_plan_destroy(self.h)
            self.h = None


def shard_cuts(block_offsets, sparse_value_offsets, K, world):
    """Panel cut points [0 = c_0 <= ... <= c_world = P] of the row-panel sharding cost model."""
    bo = np.ascontiguousarray(block_offsets, np.uint32)
    so = np.ascontiguousarray(sparse_value_offsets, np.uint32)
    P = len(bo) - 1
    cuts = np.zeros(world + 1, np.uint32)
    _check(lib().bsmr_shard_cuts(bo, so, P, K, world, cuts), "bsmr_shard_cuts")
    return cuts


def cost_cuts(block_cost, panels_per_block, P, world, prev_cuts=None, shard_ms=None):
    """bsmr_cost_cuts: row-block cuts of P panels by block costs (host only), optionally re-balanced
    by the times shard_ms[r] measured on prev_cuts (bsmr_plan_shard_rebalance's rule)."""
    bc = np.ascontiguousarray(block_cost, np.float64)
    cuts = np.zeros(world + 1, np.uint32)
    pc = None if prev_cuts is None else np.ascontiguousarray(prev_cuts, np.uint32)
    ms = None if shard_ms is None else np.ascontiguousarray(shard_ms, np.float32)
    if (pc is None) != (ms is None) or (pc is not None and (len(pc) != world + 1 or len(ms) != world)):
        raise ValueError("cost_cuts: prev_cuts (world + 1) and shard_ms (world) go together")
    ptr = (lambda a: None if a is None else a.ctypes.data)
    _check(lib().bsmr_cost_cuts(ptr(bc), len(bc), panels_per_block, P, world, ptr(pc), ptr(ms),
                                cuts), "bsmr_cost_cuts")
    return [int(c) for c in cuts]


def spmm_lists(M, N, rowptr, colidx, side, chunk, order=None):
    """bsmr_spmm_lists (host only): (segs, src, vpos) of the SpMM gather lists of side 1 (rows) or
    2 (columns). segs: (n, 4) uint32 rows {dst, first, count, part} in launch order (`order`
    first, then the other destinations ascending); src / vpos: nnz each."""
    rowptr = np.ascontiguousarray(rowptr, np.uint32)
    colidx = np.ascontiguousarray(colidx, np.uint32)
    nnz = len(colidx)
    if len(rowptr) != M + 1:
        raise ValueError("spmm_lists: rowptr needs M + 1 entries")
    ci = colidx if nnz else np.zeros(1, np.uint32)
    od = None if order is None else np.ascontiguousarray(order, np.uint32)
    optr, on = (None, 0) if od is None else (od.ctypes.data if len(od) else None, len(od))
    n = C.c_uint64()
    args = (M, N, nnz, rowptr, ci, side, chunk, optr, on)
    _check(lib().bsmr_spmm_lists(*args, None, C.byref(n), None, None), "bsmr_spmm_lists")
    segs = np.zeros((n.value, 4), np.uint32)
    src = np.zeros(max(nnz, 1), np.uint32)
    vpos = np.zeros(max(nnz, 1), np.uint32)
    _check(lib().bsmr_spmm_lists(*args, segs.ctypes.data, C.byref(n), src.ctypes.data,
                                 vpos.ctypes.data), "bsmr_spmm_lists")
    return segs, src[:nnz], vpos[:nnz]


def softmax_items(M, rowptr):
    """bsmr_softmax_items (host only): (n, 4) uint32 rows {row, first, count, kind} of the row
    softmax's item list in ascending row order. kind 1 .. 64: a packed run of `count` rows from
    `row`, lane groups of `kind` lanes; SOFTMAX_WAVE / SOFTMAX_BLOCK: one row of `count` entries."""
    rowptr = np.ascontiguousarray(rowptr, np.uint32)
    if len(rowptr) != M + 1:
        raise ValueError("softmax_items: rowptr needs M + 1 entries")
    n = C.c_uint64()
    _check(lib().bsmr_softmax_items(M, rowptr.ctypes.data, None, C.byref(n)), "bsmr_softmax_items")
    items = np.zeros((n.value, 4), np.uint32)
    _check(lib().bsmr_softmax_items(M, rowptr.ctypes.data, items.ctypes.data if n.value else None,
                                    C.byref(n)), "bsmr_softmax_items")
    return items


def softmax_limits():
    """bsmr_softmax_limits (host only): dict(wave_max, block_pass), the constants of
    Plan.softmax_stats without a plan."""
    w, b = C.c_uint32(), C.c_uint32()
    lib().bsmr_softmax_limits(C.byref(w), C.byref(b))
    return dict(wave_max=w.value, block_pass=b.value)


def attention_limits():
    """bsmr_attention_limits (host only): dict(chunk, max_row_bytes), the constants of
    Plan.attention without a plan."""
    c, b = C.c_uint32(), C.c_uint32()
    lib().bsmr_attention_limits(C.byref(c), C.byref(b))
    return dict(chunk=c.value, max_row_bytes=b.value)


def attention_backward_limits():
    """bsmr_attention_backward_limits (host only): dict(row_chunk, col_chunk, max_row_bytes), the
    constants of Plan.attention_backward without a plan."""
    r, c, b = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().bsmr_attention_backward_limits(C.byref(r), C.byref(c), C.byref(b))
    return dict(row_chunk=r.value, col_chunk=c.value, max_row_bytes=b.value)


def attention_heads_limits():
    """dict(max_batches, max_heads): BSMR_ATTENTION_MAX_BATCHES and BSMR_ATTENTION_MAX_HEADS of the
    heads calls (attention_limits() and attention_backward_limits() hold the rest)."""
    return dict(max_batches=ATTENTION_MAX_BATCHES, max_heads=ATTENTION_MAX_HEADS)


def attention_layout_check(op, batches, heads, rows, width, elem_bytes, is_output=False):
    """bsmr_attention_layout_check (host only, no device call): the layout rules of the heads calls
    for one operand (AttentionOperand.of(op); None is the null operand) of `rows` rows of `width`
    elements of `elem_bytes` bytes. Returns None when every rule holds, else the library's message
    naming the first rule that does not."""
    o = AttentionOperand.of(op)
    st = lib().bsmr_attention_layout_check(None if o is None else C.byref(o), batches, heads, rows, width, elem_bytes,
                                           1 if is_output else 0)
    return None if st == 0 else lib().bsmr_last_error().decode(errors="replace")


def sddmm_cpu(M, N, rowptr, colidx, K, A, B, threads=0):
    """bsmr_sddmm_cpu: the reference's host SDDMM (host.cpp:45-76) as product code."""
    rowptr = np.ascontiguousarray(rowptr, np.uint32)
    colidx = np.ascontiguousarray(colidx, np.uint32)
    P = np.empty(len(colidx), np.float32)
    _check(lib().bsmr_sddmm_cpu(rowptr, colidx, M, N, K, np.ascontiguousarray(A, np.float32),
                                np.ascontiguousarray(B, np.float32), P, threads), "bsmr_sddmm_cpu")
    return P


def check_rphm_arrays(M, N, rowptr, colidx, arrays, delta, verbose=True):
    """bsmr_check_rphm_arrays: the reference's check_rphm (BSMR.cpp:932-953) over host arrays.
    `arrays` maps the plan array names (ARRAYS keys) to uint32 arrays. Returns (ok, first error)."""
    a = {k: np.ascontiguousarray(v, dtype=np.uint32) for k, v in arrays.items()}
    rp = np.ascontiguousarray(rowptr, dtype=np.uint32)
    ci = np.ascontiguousarray(colidx, dtype=np.uint32)
    order = ["denseColOffsets", "denseCols", "sparseColOffsets", "sparseCols",
             "sparseValueOffsets", "blockOffsets", "blockValues", "sparseValues",
             "sparseRelativeRows", "sparseColIndices"]
    rows = a["reorderedRows"]
    st = lib().bsmr_check_rphm_arrays(M, N, len(ci), rp, ci, len(rows), rows,
                                      *[a[k] for k in order], float(delta), 1 if verbose else 0)
    if st == 0:
        return True, ""
    msg = lib().bsmr_last_error().decode(errors="replace")
    if st != CHECK_FAILED:
        raise BsmrError(f"bsmr_check_rphm_arrays failed with status {st}: {msg}")
    return False, msg


def check_data(data1, data2, verbose=False):
    """bsmr_check_data (checkData.hpp:44-79): number of mismatches; verbose prints the report."""
    a = np.ascontiguousarray(data1, np.float32)
    b = np.ascontiguousarray(data2, np.float32)
    if a.shape != b.shape:
        raise ValueError("check_data: sizes differ")
    return int(lib().bsmr_check_data(a.size, a, b, 1 if verbose else 0))
