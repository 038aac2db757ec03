"""ctypes binding of the C ABI declared in ``include/outerspace_spgemm.h``.

The shared library is built in-tree (``outerspace_amd/libouterspace_spgemm.so``) by
``make -C outerspace_amd/csrc`` / ``__graft_entry__.build()``.  There is no Python or CPU
fallback: a missing library is an ImportError, a missing GPU is an ``OspError`` at context
creation.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OSP_LIBRARY=<path> loads another build of the same ABI (`make debug` / `make ballot` write files of their own, so the
# default name is always the product build)
LIB_PATH = os.environ.get("OSP_LIBRARY") or os.path.join(_HERE, "libouterspace_spgemm.so")

OSP_F32, OSP_F64 = 0, 1
OSP_HOST, OSP_DEVICE = 0, 1
OSP_OK = 0
ERR_DIM, ERR_ARG, ERR_ALLOC, ERR_HIP, ERR_IO, ERR_RANGE, ERR_CAPACITY, ERR_UNSORTED = 1, 2, 3, 4, 5, 6, 7, 8
ERR_DUPLICATE = 233  # reference: throw(233), simulator/SimSpGEMM.cpp:49


class OspError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"[osp status {status}] {message}")
        self.status = status


class _Stats(C.Structure):
    """Base of every stats, info and descriptor struct: ``as_dict`` is the fields by name, without the ABI's ``reserved``."""

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class Config(_Stats):
    _fields_ = [("validate", C.c_int), ("partial_capacity", C.c_uint64), ("k_begin", C.c_uint64),
                ("k_end", C.c_uint64), ("row_shard_index", C.c_int), ("row_shard_count", C.c_int), ("algorithm", C.c_int),
                ("reserved", C.c_int * 5)]


class ResultInfo(_Stats):
    _fields_ = [("M", C.c_uint64), ("K", C.c_uint64), ("N", C.c_uint64),
                ("row_begin", C.c_uint64), ("row_end", C.c_uint64),
                ("nnz_a", C.c_uint64), ("nnz_b", C.c_uint64), ("nnz_c", C.c_uint64),
                ("partials", C.c_uint64), ("panels", C.c_uint32), ("light_tiles", C.c_uint64),
                ("heavy_rows", C.c_uint64), ("heavy_partials", C.c_uint64),
                ("sorted_segments", C.c_uint64), ("sorted_partials", C.c_uint64),
                ("ms_symbolic", C.c_float), ("ms_multiply", C.c_float), ("ms_merge", C.c_float),
                ("ms_compact", C.c_float), ("ms_total", C.c_float),
                ("ms_multiply_kernel", C.c_float), ("ms_merge_kernel", C.c_float), ("ms_ingest", C.c_float),
                ("multiply_launches", C.c_uint32), ("merge_launches", C.c_uint32), ("dtype", C.c_int),
                ("ms_split_kernel", C.c_float), ("split_launches", C.c_uint32), ("split_partials", C.c_uint64),
                ("dense_segments", C.c_uint64), ("direct_rows", C.c_uint64), ("direct_partials", C.c_uint64),
                ("ms_direct_plan_kernel", C.c_float), ("direct_plan_launches", C.c_uint32),
                ("rank_atomic", C.c_uint32), ("dense_atomic", C.c_uint32), ("hub_rows", C.c_uint64), ("hub_partials", C.c_uint64), ("hub_cells", C.c_uint64),
                ("ms_hub_plan_kernel", C.c_float), ("hub_plan_launches", C.c_uint32),
                ("output_slack_bytes", C.c_uint64), ("plans_overlapped", C.c_uint64),
                ("gathered_rows", C.c_uint64), ("gathered_partials", C.c_uint64), ("gathered_runs", C.c_uint64),
                ("gathered_short_partials", C.c_uint64), ("ms_expand_kernel", C.c_float), ("expand_launches", C.c_uint32),
                ("expand_partials", C.c_uint64)]


class Panel(_Stats):
    """osp_panel_t: one finished row panel of a streamed product (device pointers)."""
    _fields_ = [("row_begin", C.c_uint64), ("row_end", C.c_uint64), ("nnz", C.c_uint64),
                ("rowptr", C.c_void_p), ("colidx", C.c_void_p), ("vals", C.c_void_p),
                ("index", C.c_uint32), ("count", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class Conv2dGeometry(_Stats):
    """osp_conv2d_geometry_t"""
    _fields_ = [("kh", C.c_uint32), ("kw", C.c_uint32), ("stride_h", C.c_uint32), ("stride_w", C.c_uint32),
                ("pad_h", C.c_uint32), ("pad_w", C.c_uint32), ("dil_h", C.c_uint32), ("dil_w", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]


class MclStep(_Stats):
    """osp_mcl_step_t"""
    _fields_ = [("power", C.c_double), ("threshold", C.c_double), ("max_per_row", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class MclStats(_Stats):
    """osp_mcl_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("rows_capped", C.c_uint64), ("rows_rescued", C.c_uint64),
                ("rows_long", C.c_uint64), ("chaos", C.c_double), ("ms_total", C.c_float), ("ms_select_kernel", C.c_float),
                ("launches", C.c_uint32), ("reserved", C.c_uint32 * 5)]

class ApplyMaskStats(_Stats):
    """osp_apply_mask_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_mask", C.c_uint64), ("nnz_out", C.c_uint64), ("ms_total", C.c_float),
                ("launches", C.c_uint32), ("reserved", C.c_uint32 * 6)]

SELECT_OPS = {"lt": 0, "le": 1, "gt": 2, "ge": 3, "eq": 4, "ne": 5, "tril": 6, "triu": 7, "diag": 8, "offdiag": 9}  # osp_select_op_t


class Select(_Stats):
    """osp_select_t"""
    _fields_ = [("op", C.c_int32), ("fill", C.c_int32), ("threshold", C.c_double), ("diag", C.c_int64), ("fill_value", C.c_double),
                ("reserved", C.c_uint32 * 8)]

class SelectStats(_Stats):
    """osp_select_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("ms_total", C.c_float), ("launches", C.c_uint32),
                ("reserved", C.c_uint32 * 6)]

EWISE_MODES = {"union": 0, "intersect": 1}  # osp_ewise_mode_t
EWISE_OPS = {"plus": 0, "times": 1, "min": 2, "max": 3, "first": 4, "second": 5, "minus": 6, "div": 7}  # osp_ewise_op_t


class Ewise(_Stats):
    """osp_ewise_t"""
    _fields_ = [("mode", C.c_int32), ("op", C.c_int32), ("reserved", C.c_uint32 * 8)]


class EwiseStats(_Stats):
    """osp_ewise_stats_t"""
    _fields_ = [("nnz_a", C.c_uint64), ("nnz_b", C.c_uint64), ("nnz_both", C.c_uint64), ("nnz_out", C.c_uint64),
                ("ms_total", C.c_float), ("launches", C.c_uint32), ("reserved", C.c_uint32 * 6)]

AXES = {"rows": 0, "cols": 1}  # osp_axis_t
REDUCE_OPS = {"plus": 0, "min": 1, "max": 2, "count": 3}  # osp_reduce_op_t
VECTOR_NONE = -1  # OSP_VECTOR_NONE
# the operators of osp_vector_apply_t: osp_ewise_op_t without "first"
VECTOR_APPLY_OPS = {name: v for name, v in EWISE_OPS.items() if name != "first"}


class VectorApply(_Stats):
    """osp_vector_apply_t"""
    _fields_ = [("row_op", C.c_int32), ("col_op", C.c_int32), ("reserved", C.c_uint32 * 8)]

class VectorStats(_Stats):
    """osp_vector_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("long_segments", C.c_uint64), ("ms_total", C.c_float),
                ("launches", C.c_uint32), ("reserved", C.c_uint32 * 6)]

# the operators osp_semiring_t takes (osp_ewise_op_t values)
MXM_ADD_OPS = {name: EWISE_OPS[name] for name in ("plus", "min", "max", "first")}
MXM_MUL_OPS = {name: EWISE_OPS[name] for name in ("times", "plus", "min", "max", "first", "second")}


class Semiring(_Stats):
    """osp_semiring_t"""
    _fields_ = [("add", C.c_int32), ("mul", C.c_int32), ("reserved", C.c_uint32 * 8)]


class MxmStats(_Stats):
    """osp_mxm_stats_t"""
    _fields_ = [("nnz_a", C.c_uint64), ("nnz_b", C.c_uint64), ("products", C.c_uint64), ("nnz_out", C.c_uint64),
                ("short_rows", C.c_uint64), ("long_rows", C.c_uint64), ("batches", C.c_uint32), ("launches", C.c_uint32),
                ("ms_total", C.c_float), ("reserved", C.c_uint32 * 7)]


class MxmMaskedStats(_Stats):
    """osp_mxm_masked_stats_t"""
    _fields_ = [("nnz_a", C.c_uint64), ("nnz_b", C.c_uint64), ("nnz_mask", C.c_uint64), ("products", C.c_uint64),
                ("products_kept", C.c_uint64), ("nnz_out", C.c_uint64), ("short_rows", C.c_uint64), ("long_rows", C.c_uint64),
                ("batches", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float), ("reserved", C.c_uint32 * 7)]

# the add operators osp_csr_mxv takes: the value operators of osp_csr_reduce (mul: MXM_MUL_OPS)
MXV_ADD_OPS = {name: EWISE_OPS[name] for name in ("plus", "min", "max")}


class MxvStats(_Stats):
    """osp_mxv_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("long_segments", C.c_uint64), ("group", C.c_uint32),
                ("launches", C.c_uint32), ("ms_total", C.c_float), ("reserved", C.c_uint32 * 7)]

# the add operators osp_csr_mxv_arg takes: the two of MXV_ADD_OPS under which a product has a position (mul: MXM_MUL_OPS)
MXV_ARG_ADD_OPS = {name: EWISE_OPS[name] for name in ("min", "max")}


class MxvArgStats(_Stats):
    """osp_mxv_arg_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("long_segments", C.c_uint64), ("rows_without", C.c_uint64),
                ("group", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float), ("reserved", C.c_uint32 * 7)]

MXD_MAX_COLS = 65536   # OSP_MXD_MAX_COLS


class MxdStats(_Stats):
    """osp_mxd_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("cols", C.c_uint64), ("long_segments", C.c_uint64),
                ("lanes_per_row", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float), ("reserved", C.c_uint32 * 7)]

# the accum operators osp_csr_sddmm takes: osp_csr_apply_vectors' table (None passes VECTOR_NONE, which means "second")
SDDMM_ACCUM_OPS = VECTOR_APPLY_OPS


class SddmmStats(_Stats):
    """osp_sddmm_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("cols", C.c_uint64), ("lanes_per_entry", C.c_uint32),
                ("launches", C.c_uint32), ("ms_total", C.c_float), ("reserved", C.c_uint32 * 7)]

class Transpose(_Stats):
    """osp_transpose_t"""
    _fields_ = [("reserved", C.c_uint32 * 8)]


class TransposeStats(_Stats):
    """osp_transpose_stats_t"""
    _fields_ = [("nnz", C.c_uint64), ("path", C.c_uint32), ("passes", C.c_uint32), ("launches", C.c_uint32), ("ms_total", C.c_float),
                ("reserved", C.c_uint32 * 6)]

class Extract(_Stats):
    """osp_extract_t"""
    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("n_cols", C.c_uint64), ("space", C.c_int32),
                ("reserved", C.c_uint32 * 7)]


class ExtractStats(_Stats):
    """osp_extract_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_gathered", C.c_uint64), ("nnz_out", C.c_uint64), ("ms_total", C.c_float),
                ("launches", C.c_uint32), ("readbacks", C.c_uint32), ("reserved", C.c_uint32 * 5)]

DUP_OPS = {"error": 0, "plus": 1, "min": 2, "max": 3, "first": 4, "last": 5, "count": 6}  # osp_dup_op_t


class Build(_Stats):
    """osp_build_t"""
    _fields_ = [("M", C.c_uint64), ("N", C.c_uint64), ("nnz", C.c_uint64), ("rows", C.c_void_p), ("cols", C.c_void_p), ("vals", C.c_void_p),
                ("dtype", C.c_int32), ("space", C.c_int32), ("dup", C.c_int32), ("reserved", C.c_uint32 * 7)]


class BuildStats(_Stats):
    """osp_build_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("long_runs", C.c_uint64), ("ms_total", C.c_float),
                ("launches", C.c_uint32), ("readbacks", C.c_uint32), ("reserved", C.c_uint32 * 5)]

ASSIGN_NO_ACCUM = -1  # OSP_ASSIGN_NO_ACCUM
# the accum operators osp_csr_assign takes: the union's (None passes ASSIGN_NO_ACCUM: the region is replaced)
ASSIGN_ACCUM_OPS = {name: EWISE_OPS[name] for name in ("plus", "times", "min", "max", "first", "second")}


class Assign(_Stats):
    """osp_assign_t"""
    _fields_ = [("rows", C.c_void_p), ("n_rows", C.c_uint64), ("cols", C.c_void_p), ("n_cols", C.c_uint64), ("space", C.c_int32),
                ("accum", C.c_int32), ("reserved", C.c_uint32 * 6)]


class AssignStats(_Stats):
    """osp_assign_stats_t"""
    _fields_ = [("nnz_c", C.c_uint64), ("nnz_a", C.c_uint64), ("nnz_region", C.c_uint64), ("nnz_both", C.c_uint64),
                ("nnz_out", C.c_uint64), ("ms_total", C.c_float), ("launches", C.c_uint32), ("readbacks", C.c_uint32),
                ("reserved", C.c_uint32 * 5)]

# the operators osp_csr_kron takes: the mul operators of a semiring
KRON_OPS = MXM_MUL_OPS
KRON_LAUNCHES = 2  # OSP_KRON_LAUNCHES


class Kron(_Stats):
    """osp_kron_t"""
    _fields_ = [("op", C.c_int32), ("reserved", C.c_uint32 * 7)]


class KronStats(_Stats):
    """osp_kron_stats_t"""
    _fields_ = [("nnz_a", C.c_uint64), ("nnz_b", C.c_uint64), ("nnz_out", C.c_uint64), ("ms_total", C.c_float),
                ("launches", C.c_uint32), ("readbacks", C.c_uint32), ("reserved", C.c_uint32 * 5)]

SELECT_K_ORDERS = {"largest": 0, "smallest": 1, "random": 2}  # osp_select_k_order_t


class SelectK(_Stats):
    """osp_select_k_t"""
    _fields_ = [("order", C.c_int32), ("k", C.c_uint32), ("seed", C.c_uint64), ("reserved", C.c_uint32 * 8)]


class SelectKStats(_Stats):
    """osp_select_k_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("rows_capped", C.c_uint64), ("rows_long", C.c_uint64),
                ("ms_total", C.c_float), ("launches", C.c_uint32), ("readbacks", C.c_uint32), ("reserved", C.c_uint32 * 6)]


# capped rows of a k-select longer than this are selected by a workgroup, shorter ones by one wave (kSelectKLongMin, osp_select_k.h)
SELECT_K_LONG_MIN = 2048

SCAN_OPS = {"plus": 0, "min": 1, "max": 2}  # the osp_reduce_op_t values osp_csr_scan takes
SCAN_BLOCK = 32        # OSP_SCAN_BLOCK: entries of one block of the scan order
SCAN_CHAIN_LANE = 16   # rows of more blocks than this are chained by a whole wave (kScanChainLane, osp_scan.h)
SCAN_LOCAL_TILE = 128  # blocks of one workgroup of the scan's local pass (kScanLocalThreads, osp_scan.h)


class Scan(_Stats):
    """osp_scan_t"""
    _fields_ = [("op", C.c_int32), ("reserved", C.c_uint32 * 8)]


class ScanStats(_Stats):
    """osp_scan_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("blocks", C.c_uint64), ("ms_total", C.c_float),
                ("launches", C.c_uint32), ("readbacks", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class Draw(_Stats):
    """osp_draw_t"""
    _fields_ = [("draws", C.c_uint32), ("reserved0", C.c_uint32), ("seed", C.c_uint64), ("reserved", C.c_uint32 * 8)]


class DrawStats(_Stats):
    """osp_draw_stats_t"""
    _fields_ = [("nnz_in", C.c_uint64), ("nnz_out", C.c_uint64), ("rows_without", C.c_uint64), ("ms_total", C.c_float),
                ("launches", C.c_uint32), ("readbacks", C.c_uint32), ("reserved", C.c_uint32 * 7)]


PANEL_FN = C.CFUNCTYPE(C.c_int, C.POINTER(Panel), C.c_void_p)

MULTI_MAX_RANKS = 16


class MultiRankInfo(_Stats):
    """osp_multi_rank_info_t"""
    _fields_ = [("device", C.c_int), ("k_begin", C.c_uint64), ("k_end", C.c_uint64), ("row_begin", C.c_uint64), ("row_end", C.c_uint64),
                ("partials_local", C.c_uint64), ("records_received", C.c_uint64), ("bytes_sent", C.c_uint64), ("nnz_c", C.c_uint64),
                ("ms_symbolic", C.c_float), ("ms_multiply_kernel", C.c_float), ("ms_merge", C.c_float), ("ms_total", C.c_float),
                ("bytes_to", C.c_uint64 * MULTI_MAX_RANKS), ("copy_streams", C.c_int), ("max_copies_outstanding", C.c_int),
                ("max_copies_in_flight", C.c_int), ("ms_exchange", C.c_float)]


class MultiInfo(_Stats):
    """osp_multi_info_t"""
    _fields_ = [("nranks", C.c_int), ("subpanels", C.c_int), ("M", C.c_uint64), ("K", C.c_uint64), ("N", C.c_uint64),
                ("nnz_c", C.c_uint64), ("partials", C.c_uint64), ("bytes_exchanged", C.c_uint64), ("ms_total", C.c_float),
                ("ms_upload", C.c_float), ("rank", MultiRankInfo * MULTI_MAX_RANKS)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "rank"}
        d["ranks"] = [{n: (list(getattr(self.rank[g], n))[:self.nranks] if n == "bytes_to" else getattr(self.rank[g], n))
                       for n, _ in MultiRankInfo._fields_} for g in range(self.nranks)]
        return d


# every symbol include/outerspace_spgemm.h declares
EXPORTS = [
    "osp_context_create", "osp_context_create_on_stream", "osp_context_destroy", "osp_context_trim",
    "osp_config_default", "osp_last_error_string", "osp_status_string", "osp_spgemm_csc_csr", "osp_spgemm_csc_csr_panels",
    "osp_spgemm_coo", "osp_spgemm_csc_csr_aos", "osp_context_alloc", "osp_context_free",
    "osp_spgemm_partials", "osp_result_partials", "osp_merge_record_parts",
    "osp_merge_csr_parts", "osp_result_info", "osp_result_copy_csr", "osp_result_device_ptrs",
    "osp_result_destroy", "osp_mtx_read", "osp_host_free", "osp_coo_to_compressed_f32",
    "osp_coo_to_compressed_f64", "osp_spgemm_mtx", "osp_result_write_mtx", "osp_csr_bias_relu", "osp_result_coo_rows",
    "osp_stream_copy_probe", "osp_im2col_csc", "osp_spgemm_conv2d", "osp_csr_maxpool2d",
    "osp_multi_context_create", "osp_multi_context_destroy", "osp_multi_operands_create", "osp_multi_operands_destroy", "osp_spgemm_multi",
    "osp_spgemm_csc_csr_multi", "osp_multi_result_info", "osp_multi_result_shard", "osp_multi_result_copy_csr", "osp_multi_result_destroy",
]

# every symbol include/outerspace_spgemm_masked.h declares (kept apart from EXPORTS: that list pins outerspace_spgemm.h)
MASKED_EXPORTS = ["osp_spgemm_masked"]

# every symbol include/outerspace_spgemm_mcl.h declares
MCL_EXPORTS = ["osp_csr_inflate_prune"]

# every symbol include/outerspace_spgemm_apply_mask.h declares
APPLY_MASK_EXPORTS = ["osp_csr_apply_mask"]

# every symbol include/outerspace_spgemm_select.h declares
SELECT_EXPORTS = ["osp_csr_select"]

# every symbol include/outerspace_spgemm_ewise.h declares
EWISE_EXPORTS = ["osp_csr_ewise"]

# every symbol include/outerspace_spgemm_vector.h declares
VECTOR_EXPORTS = ["osp_csr_reduce", "osp_csr_apply_vectors", "osp_csr_select_vertices"]

# every symbol include/outerspace_spgemm_mxm.h declares
MXM_EXPORTS = ["osp_csr_mxm"]

# every symbol include/outerspace_spgemm_mxm_masked.h declares
MXM_MASKED_EXPORTS = ["osp_csr_mxm_masked"]

# every symbol include/outerspace_spgemm_transpose.h declares
TRANSPOSE_EXPORTS = ["osp_csr_transpose"]

# every symbol include/outerspace_spgemm_mxv.h declares
MXV_EXPORTS = ["osp_csr_mxv"]

# every symbol include/outerspace_spgemm_mxv_arg.h declares
MXV_ARG_EXPORTS = ["osp_csr_mxv_arg"]

# every symbol include/outerspace_spgemm_mxd.h declares
MXD_EXPORTS = ["osp_csr_mxd"]

# every symbol include/outerspace_spgemm_sddmm.h declares
SDDMM_EXPORTS = ["osp_csr_sddmm"]

# every symbol include/outerspace_spgemm_extract.h declares
EXTRACT_EXPORTS = ["osp_csr_extract"]

# every symbol include/outerspace_spgemm_build.h declares
BUILD_EXPORTS = ["osp_csr_build"]

# every symbol include/outerspace_spgemm_assign.h declares
ASSIGN_EXPORTS = ("osp_csr_assign",)

# every symbol include/outerspace_spgemm_kron.h declares
KRON_EXPORTS = ("osp_csr_kron",)

# every symbol include/outerspace_spgemm_select_k.h declares
SELECT_K_EXPORTS = ("osp_csr_select_k",)

# every symbol include/outerspace_spgemm_scan.h declares
SCAN_EXPORTS = ("osp_csr_scan", "osp_csr_draw")

_lib = None


def lib():
    """Load the library (once).  Raises ImportError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `make -C outerspace_amd/csrc` "
                          "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                          "There is no CPU fallback.")
    # One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64 (SONAME libamdhip64.so.7, asked for as
    # "libamdhip64.so" by torch's libraries): loaded first, it also satisfies this library's NEEDED entry; loaded second,
    # the process ends up with two runtimes and torch reports "No HIP GPUs are available".  The package uses torch for
    # device memory anyway, so it goes first when it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.osp_last_error_string.restype = C.c_char_p
    L.osp_status_string.restype = C.c_char_p
    L.osp_status_string.argtypes = [i32]
    L.osp_context_create.argtypes = [i32, C.POINTER(vp)]
    L.osp_context_create_on_stream.argtypes = [i32, vp, C.POINTER(vp)]
    L.osp_context_destroy.argtypes = [vp]
    L.osp_context_trim.argtypes = [vp]
    L.osp_context_alloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.osp_context_free.argtypes = [vp, vp]
    L.osp_spgemm_csc_csr_aos.argtypes = [vp, i32, u64, u64, u64, vp, vp, vp, vp, i32, C.POINTER(Config), C.POINTER(vp)]
    L.osp_config_default.argtypes = [C.POINTER(Config)]
    L.osp_config_default.restype = None
    L.osp_spgemm_csc_csr.argtypes = [vp, i32, u64, u64, u64, vp, vp, vp, vp, vp, vp, i32,
                                     C.POINTER(Config), C.POINTER(vp)]
    L.osp_spgemm_csc_csr_panels.argtypes = [vp, i32, u64, u64, u64, vp, vp, vp, vp, vp, vp, i32, C.POINTER(Config), PANEL_FN, vp,
                                            C.POINTER(ResultInfo)]
    L.osp_spgemm_coo.argtypes = [vp, i32, u64, u64, u64, u64, vp, vp, vp, u64, vp, vp, vp, i32, C.POINTER(Config), C.POINTER(vp)]
    L.osp_spgemm_partials.argtypes = [vp, i32, u64, u64, u64, vp, vp, vp, vp, vp, vp, i32, C.POINTER(Config), C.POINTER(vp)]
    L.osp_result_partials.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.osp_merge_record_parts.argtypes = [vp, i32, u64, u64, i32, C.POINTER(vp), C.POINTER(vp), i32, C.POINTER(Config), C.POINTER(vp)]
    L.osp_merge_csr_parts.argtypes = [vp, i32, u64, u64, i32, C.POINTER(vp), C.POINTER(vp),
                                      C.POINTER(vp), i32, C.POINTER(Config), C.POINTER(vp)]
    L.osp_result_info.argtypes = [vp, C.POINTER(ResultInfo)]
    L.osp_result_copy_csr.argtypes = [vp, vp, vp, vp, i32]
    L.osp_result_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.osp_result_destroy.argtypes = [vp]
    L.osp_mtx_read.argtypes = [C.c_char_p, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64),
                               C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.osp_host_free.argtypes = [vp]
    L.osp_host_free.restype = None
    for sfx in ("f32", "f64"):
        getattr(L, f"osp_coo_to_compressed_{sfx}").argtypes = [i32, u64, u64, vp, vp, vp, vp, vp, vp]
    L.osp_spgemm_mtx.argtypes = [vp, i32, C.c_char_p, C.c_char_p, i32, C.POINTER(Config), C.POINTER(vp)]
    L.osp_result_write_mtx.argtypes = [vp, C.c_char_p]
    L.osp_stream_copy_probe.argtypes = [vp, u64, i32, C.POINTER(C.c_double)]
    L.osp_multi_context_create.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
    L.osp_multi_context_destroy.argtypes = [vp]
    L.osp_multi_operands_create.argtypes = [vp, i32, u64, u64, u64, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.osp_multi_operands_destroy.argtypes = [vp]
    L.osp_spgemm_multi.argtypes = [vp, vp, C.POINTER(Config), C.POINTER(vp)]
    L.osp_spgemm_csc_csr_multi.argtypes = [C.POINTER(i32), i32, i32, u64, u64, u64, vp, vp, vp, vp, vp, vp, C.POINTER(Config), C.POINTER(vp),
                                           C.POINTER(vp)]
    L.osp_multi_result_info.argtypes = [vp, C.POINTER(MultiInfo)]
    L.osp_multi_result_shard.argtypes = [vp, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(vp)]
    L.osp_multi_result_copy_csr.argtypes = [vp, vp, vp, vp]
    L.osp_multi_result_destroy.argtypes = [vp]
    L.osp_csr_bias_relu.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    L.osp_result_coo_rows.argtypes = [vp, vp]
    L.osp_im2col_csc.argtypes = [vp, i32, u64, u64, u64, u64, u64, vp, vp, vp, i32, C.POINTER(Conv2dGeometry), i32, C.POINTER(u64),
                                 vp, vp, vp]
    L.osp_spgemm_conv2d.argtypes = [vp, i32, u64, u64, u64, u64, u64, vp, vp, vp, u64, u64, vp, vp, vp, i32, C.POINTER(Conv2dGeometry),
                                    C.POINTER(Config), C.POINTER(vp)]
    u32 = C.c_uint32
    L.osp_csr_maxpool2d.argtypes = [vp, u64, u64, u64, u32, u32, u32, u32, C.POINTER(vp)]
    L.osp_spgemm_masked.argtypes = [vp, i32, u64, u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(Config), C.POINTER(vp)]
    L.osp_csr_inflate_prune.argtypes = [vp, C.POINTER(MclStep), i32, C.POINTER(vp), C.POINTER(MclStats)]
    L.osp_csr_apply_mask.argtypes = [vp, u64, u64, vp, vp, i32, i32, i32, C.POINTER(vp), C.POINTER(ApplyMaskStats)]
    L.osp_csr_select.argtypes = [vp, C.POINTER(Select), C.POINTER(vp), C.POINTER(SelectStats)]
    L.osp_csr_ewise.argtypes = [vp, vp, C.POINTER(Ewise), C.POINTER(vp), C.POINTER(EwiseStats)]
    L.osp_csr_reduce.argtypes = [vp, i32, i32, vp, i32, C.POINTER(VectorStats)]
    L.osp_csr_apply_vectors.argtypes = [vp, C.POINTER(VectorApply), vp, vp, i32, C.POINTER(vp), C.POINTER(VectorStats)]
    L.osp_csr_select_vertices.argtypes = [vp, vp, vp, i32, C.POINTER(vp), C.POINTER(VectorStats)]
    L.osp_csr_mxm.argtypes = [vp, vp, C.POINTER(Semiring), C.POINTER(vp), C.POINTER(MxmStats)]
    L.osp_csr_mxm_masked.argtypes = [vp, vp, vp, i32, C.POINTER(Semiring), C.POINTER(vp), C.POINTER(MxmMaskedStats)]
    L.osp_csr_transpose.argtypes = [vp, C.POINTER(Transpose), C.POINTER(vp), C.POINTER(TransposeStats)]
    L.osp_csr_mxv.argtypes = [vp, C.POINTER(Semiring), vp, vp, i32, C.POINTER(MxvStats)]
    L.osp_csr_mxv_arg.argtypes = [vp, C.POINTER(Semiring), vp, vp, vp, i32, C.POINTER(MxvArgStats)]
    L.osp_csr_mxd.argtypes = [vp, C.POINTER(Semiring), vp, u64, vp, i32, C.POINTER(MxdStats)]
    L.osp_csr_sddmm.argtypes = [vp, C.POINTER(Semiring), i32, vp, vp, u64, i32, C.POINTER(vp), C.POINTER(SddmmStats)]
    L.osp_csr_extract.argtypes = [vp, C.POINTER(Extract), C.POINTER(vp), C.POINTER(ExtractStats)]
    L.osp_csr_build.argtypes = [vp, C.POINTER(Build), C.POINTER(vp), C.POINTER(BuildStats)]
    L.osp_csr_assign.argtypes = [vp, vp, C.POINTER(Assign), C.POINTER(vp), C.POINTER(AssignStats)]
    L.osp_csr_kron.argtypes = [vp, vp, C.POINTER(Kron), C.POINTER(vp), C.POINTER(KronStats)]
    L.osp_csr_select_k.argtypes = [vp, C.POINTER(SelectK), C.POINTER(vp), C.POINTER(SelectKStats)]
    L.osp_csr_scan.argtypes = [vp, C.POINTER(Scan), C.POINTER(vp), C.POINTER(ScanStats)]
    L.osp_csr_draw.argtypes = [vp, C.POINTER(Draw), vp, vp, i32, C.POINTER(DrawStats)]
    _lib = L
    return L


def check(status):
    if status != OSP_OK:
        raise OspError(status, lib().osp_last_error_string().decode(errors="replace"))
