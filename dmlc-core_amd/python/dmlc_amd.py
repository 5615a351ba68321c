"""Python binding of the MI355X parse path (ctypes over include/dmlc_amd.h).

PyTorch is used only as plumbing: device buffers (torch.cuda tensors) and the
current HIP stream.  All parsing runs in libdmlc_amd.so's HIP kernels; there is
no CPU fallback -- importing this module on a machine without the built
library, or calling parse() without a GPU, raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DMLC_AMD_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libdmlc_amd.so")

LIBSVM, CSV, LIBFM = 0, 1, 2
F32, I32, I64 = 0, 1, 2
ROWS, INDEX, VALUE, WEIGHT, QID, LABEL, FIELD = range(7)
FLAG_COUNT_ONLY = 1
FLAG_FILL_ONLY = 2
FLAG_EXACT = 4
FLAG_MAX_INDEX = 8  # result.max_index / max_field (RowBlockContainer::max_index, NumCol)
ERR_CAPACITY = 16
_FMT = {"libsvm": LIBSVM, "csv": CSV, "libfm": LIBFM}
_VT = {"f32": F32, "float32": F32, "i32": I32, "int32": I32, "i64": I64, "int64": I64}


class Params(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("index_bits", ctypes.c_int32),
                ("value_type", ctypes.c_int32), ("indexing_mode", ctypes.c_int32),
                ("label_column", ctypes.c_int32), ("weight_column", ctypes.c_int32),
                ("delimiter", ctypes.c_int32), ("tile_bytes", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("nthread", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 2)]


class Csr(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_void_p), ("label", ctypes.c_void_p), ("weight", ctypes.c_void_p),
                ("qid", ctypes.c_void_p), ("field", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("value", ctypes.c_void_p), ("cap", ctypes.c_uint64 * 8)]


class DenseParams(ctypes.Structure):
    """dmlc_amd_dense_params (64 bytes)."""
    _fields_ = [("index_bits", ctypes.c_int32), ("value_type", ctypes.c_int32),
                ("row_begin", ctypes.c_uint64), ("max_rows", ctypes.c_uint64), ("ncol", ctypes.c_uint64),
                ("ld", ctypes.c_uint64), ("fill_bits", ctypes.c_uint64),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class Cuts(ctypes.Structure):
    """dmlc_amd_cuts (24 bytes)."""
    _fields_ = [("cut_ptr", ctypes.c_void_p), ("cut_value", ctypes.c_void_p), ("n_cuts", ctypes.c_uint64)]


class BinsParams(ctypes.Structure):
    """dmlc_amd_bins_params (64 bytes)."""
    _fields_ = [("index_bits", ctypes.c_int32), ("value_type", ctypes.c_int32), ("code_bytes", ctypes.c_int32),
                ("missing_code", ctypes.c_uint32),
                ("row_begin", ctypes.c_uint64), ("max_rows", ctypes.c_uint64), ("ncol", ctypes.c_uint64),
                ("ld", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class GatherParams(ctypes.Structure):
    """dmlc_amd_gather_params (32 bytes)."""
    _fields_ = [("index_bits", ctypes.c_int32), ("value_type", ctypes.c_int32), ("label_type", ctypes.c_int32),
                ("id_bits", ctypes.c_int32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class CscParams(ctypes.Structure):
    """dmlc_amd_csc_params (56 bytes)."""
    _fields_ = [("index_bits", ctypes.c_int32), ("value_type", ctypes.c_int32),
                ("row_begin", ctypes.c_uint64), ("max_rows", ctypes.c_uint64), ("ncol", ctypes.c_uint64),
                ("max_entries", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class Csc(ctypes.Structure):
    """dmlc_amd_csc."""
    _fields_ = [("col_offset", ctypes.c_void_p), ("row", ctypes.c_void_p), ("value", ctypes.c_void_p),
                ("pos", ctypes.c_void_p), ("cap", ctypes.c_uint64)]


class CutsOut(ctypes.Structure):
    """dmlc_amd_cuts_out (24 bytes): dmlc_amd_cuts's layout, cap in n_cuts's place."""
    _fields_ = [("cut_ptr", ctypes.c_void_p), ("cut_value", ctypes.c_void_p), ("cap", ctypes.c_uint64)]


class MakeCutsParams(ctypes.Structure):
    """dmlc_amd_make_cuts_params (56 bytes)."""
    _fields_ = [("index_bits", ctypes.c_int32), ("value_type", ctypes.c_int32),
                ("row_begin", ctypes.c_uint64), ("max_rows", ctypes.c_uint64), ("ncol", ctypes.c_uint64),
                ("max_entries", ctypes.c_uint64), ("max_bin", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


# d_status words 4 - 6 of dmlc_amd_make_cuts (0 - 3 and the flag bits are to_csc's)
CUTS_NAN, CUTS_N_CUTS, CUTS_EMPTY_COLS = 4, 5, 6

# d_status words of dmlc_amd_to_csc and its flag bits
CSC_KEPT, CSC_DROPPED, CSC_FIRST, CSC_FLAGS = range(4)
CSC_FLAG_ERROR, CSC_FLAG_VALUE_COUNT, CSC_FLAG_OFFSET_CAP, CSC_FLAG_CAPACITY, CSC_FLAG_MAX_ENTRIES = 1, 2, 4, 8, 16

# d_status words of dmlc_amd_gather_rows and its flag bits
GATHER_ROWS, GATHER_BAD, GATHER_FIRST, GATHER_FLAGS = range(4)
GATHER_FLAG_ERROR, GATHER_FLAG_COUNT, GATHER_FLAG_OFFSET_CAP, GATHER_FLAG_CAPACITY = 1, 2, 4, 8

# d_status words of dmlc_amd_to_dense and its flag bits
DENSE_ROWS, DENSE_DROPPED, DENSE_FIRST, DENSE_FLAGS = range(4)
DENSE_FLAG_ERROR, DENSE_FLAG_VALUE_COUNT, DENSE_FLAG_OFFSET_CAP, DENSE_FLAG_ROW_TOO_LONG = 1, 2, 4, 8

# d_status words of dmlc_amd_to_bins (0 - 3 and flag bits 0 - 3 as the dense ones) and its own flag bits
BINS_ROWS, BINS_DROPPED, BINS_FIRST, BINS_FLAGS, BINS_NAN, BINS_UNBINNED = range(6)
BINS_FLAG_CODE_RANGE, BINS_FLAG_CUT_PTR = 16, 32
BINS_GLOBAL = 1

_LIB = None


def lib():
    """Load libdmlc_amd.so; raises if it was not built (no silent fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libdmlc_amd.so not built: run `make -C dmlc-core_amd` "
                               "(or __graft_entry__.build())")
        # One HIP runtime per process: PyTorch ships its own libamdhip64; load
        # it first so this library binds to the same runtime (loaded the other
        # way round, two runtimes coexist and the second sees no device).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        L.dmlc_amd_workspace_bytes.restype = ctypes.c_size_t
        L.dmlc_amd_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(Params)]
        L.dmlc_amd_parse.restype = ctypes.c_int
        L.dmlc_amd_parse.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.POINTER(Params), ctypes.POINTER(Csr), ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
        L.dmlc_amd_error_string.restype = ctypes.c_char_p
        L.dmlc_amd_error_string.argtypes = [ctypes.c_int]
        L.dmlc_amd_device_count.restype = ctypes.c_int
        L.dmlc_amd_abi_version.restype = ctypes.c_int
        if hasattr(L, "dmlc_amd_build_id"):  # (A/B variant libraries built from older sources lack it)
            L.dmlc_amd_build_id.restype = ctypes.c_char_p
        L.dmlc_amd_strtof_batch.restype = ctypes.c_int
        L.dmlc_amd_strtof_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p]
        L.dmlc_amd_last_hip_error.restype = ctypes.c_char_p
        L.dmlc_amd_copy.restype = ctypes.c_int
        L.dmlc_amd_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        if hasattr(L, "dmlc_amd_copy_n"):  # (absent from older diagnostic variant builds)
            L.dmlc_amd_copy_n.restype = ctypes.c_int
            L.dmlc_amd_copy_n.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_void_p]
        if hasattr(L, "dmlc_amd_fast_geometry"):  # (A/B builds of older sources lack it)
            L.dmlc_amd_fast_geometry.restype = ctypes.c_int
            L.dmlc_amd_fast_geometry.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "dmlc_amd_to_dense"):  # (A/B builds of older sources lack it)
            L.dmlc_amd_to_dense.restype = ctypes.c_int
            L.dmlc_amd_to_dense.argtypes = [ctypes.POINTER(Csr), ctypes.c_void_p, ctypes.POINTER(DenseParams),
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            L.dmlc_amd_dense_geometry.restype = ctypes.c_int
            L.dmlc_amd_dense_geometry.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "dmlc_amd_gather_rows"):  # (A/B builds of older sources lack it)
            L.dmlc_amd_gather_workspace_bytes.restype = ctypes.c_size_t
            L.dmlc_amd_gather_workspace_bytes.argtypes = [ctypes.c_uint64]
            L.dmlc_amd_gather_rows.restype = ctypes.c_int
            L.dmlc_amd_gather_rows.argtypes = [ctypes.POINTER(Csr), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.POINTER(GatherParams), ctypes.POINTER(Csr), ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
            L.dmlc_amd_gather_geometry.restype = ctypes.c_int
            L.dmlc_amd_gather_geometry.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "dmlc_amd_to_csc"):  # (A/B builds of older sources lack it)
            L.dmlc_amd_csc_workspace_bytes.restype = ctypes.c_size_t
            L.dmlc_amd_csc_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(CscParams)]
            L.dmlc_amd_to_csc.restype = ctypes.c_int
            L.dmlc_amd_to_csc.argtypes = [ctypes.POINTER(Csr), ctypes.c_void_p, ctypes.POINTER(CscParams),
                                          ctypes.POINTER(Csc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p]
            L.dmlc_amd_csc_geometry.restype = ctypes.c_int
            L.dmlc_amd_csc_geometry.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "dmlc_amd_to_bins"):  # (A/B builds of older sources lack it)
            L.dmlc_amd_to_bins.restype = ctypes.c_int
            L.dmlc_amd_to_bins.argtypes = [ctypes.POINTER(Csr), ctypes.c_void_p, ctypes.POINTER(Cuts),
                                           ctypes.POINTER(BinsParams), ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p]
            L.dmlc_amd_bins_geometry.restype = ctypes.c_int
            L.dmlc_amd_bins_geometry.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        if hasattr(L, "dmlc_amd_make_cuts"):  # (A/B builds of older sources lack it)
            L.dmlc_amd_make_cuts_workspace_bytes.restype = ctypes.c_size_t
            L.dmlc_amd_make_cuts_workspace_bytes.argtypes = [ctypes.c_uint64, ctypes.c_uint64,
                                                             ctypes.POINTER(MakeCutsParams)]
            L.dmlc_amd_make_cuts.restype = ctypes.c_int
            L.dmlc_amd_make_cuts.argtypes = [ctypes.POINTER(Csr), ctypes.c_void_p, ctypes.POINTER(MakeCutsParams),
                                             ctypes.POINTER(CutsOut), ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.c_void_p]
            L.dmlc_amd_make_cuts_geometry.restype = ctypes.c_int
            L.dmlc_amd_make_cuts_geometry.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.dmlc_amd_profile_begin.restype = ctypes.c_int
        L.dmlc_amd_profile_end.restype = ctypes.c_int
        L.dmlc_amd_profile_end.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                           ctypes.POINTER(ctypes.c_char_p)]
        _LIB = L
    return _LIB


def profile_begin():
    lib().dmlc_amd_profile_begin()


def profile_end():
    """-> (summed kernel ms, launches, kernel name) since profile_begin()."""
    t, n, k = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_char_p()
    if lib().dmlc_amd_profile_end(ctypes.byref(t), ctypes.byref(n), ctypes.byref(k)) != 0:
        raise RuntimeError("dmlc_amd_profile_end failed")
    return t.value, n.value, (k.value or b"").decode()


EXPORTED_SYMBOLS = ("dmlc_amd_parse", "dmlc_amd_workspace_bytes", "dmlc_amd_error_string",
                    "dmlc_amd_device_count", "dmlc_amd_abi_version", "dmlc_amd_strtof_batch",
                    "dmlc_amd_profile_begin", "dmlc_amd_profile_end", "dmlc_amd_last_hip_error",
                    "dmlc_amd_copy", "dmlc_amd_copy_n", "dmlc_amd_copy_n_dev", "dmlc_amd_fast_geometry",
                    "dmlc_amd_build_id", "dmlc_amd_to_dense", "dmlc_amd_dense_geometry", "dmlc_amd_gather_rows",
                    "dmlc_amd_gather_workspace_bytes", "dmlc_amd_gather_geometry", "dmlc_amd_to_csc",
                    "dmlc_amd_csc_workspace_bytes", "dmlc_amd_csc_geometry", "dmlc_amd_to_bins",
                    "dmlc_amd_bins_geometry", "dmlc_amd_make_cuts", "dmlc_amd_make_cuts_workspace_bytes",
                    "dmlc_amd_make_cuts_geometry")


def csc_geometry():
    """(entries per tile, bits per digit pass) of dmlc_amd_to_csc in the loaded
    library (dmlc_amd_csc_geometry)."""
    t, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().dmlc_amd_csc_geometry(ctypes.byref(t), ctypes.byref(b))
    return int(t.value), int(b.value)


def make_cuts_geometry():
    """(entries per tile, bits per digit pass) of dmlc_amd_make_cuts in the
    loaded library (dmlc_amd_make_cuts_geometry)."""
    t, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().dmlc_amd_make_cuts_geometry(ctypes.byref(t), ctypes.byref(b))
    return int(t.value), int(b.value)


def dense_geometry():
    """(cells per tile, most rows per tile) of dmlc_amd_to_dense in the loaded
    library: a workgroup owns S = min(ncol, cells) columns of min(rows, cells
    // S) rows (dmlc_amd_dense_geometry)."""
    c, r = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().dmlc_amd_dense_geometry(ctypes.byref(c), ctypes.byref(r))
    return int(c.value), int(r.value)


def bins_geometry():
    """(cells per tile, most rows per tile) of dmlc_amd_to_bins in the loaded
    library, read as dense_geometry()'s (dmlc_amd_bins_geometry)."""
    c, r = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().dmlc_amd_bins_geometry(ctypes.byref(c), ctypes.byref(r))
    return int(c.value), int(r.value)


def gather_geometry():
    """Ids per tile (one workgroup) of dmlc_amd_gather_rows in the loaded
    library (dmlc_amd_gather_geometry)."""
    r = ctypes.c_uint32(0)
    lib().dmlc_amd_gather_geometry(ctypes.byref(r))
    return int(r.value)


def fill_bits_of(fill, value_type):
    """Bit pattern of `fill` as the value type (F32 | I32 | I64)."""
    if value_type == F32:
        return int(np.array([fill], dtype=np.float32).view(np.uint32)[0])
    if isinstance(fill, float) and fill != fill:
        raise ValueError("an integer value type has no NaN: pass fill= or fill_bits=")
    if value_type == I32:
        return int(np.array([fill], dtype=np.int32).view(np.uint32)[0])
    return int(np.array([fill], dtype=np.int64).view(np.uint64)[0])


def fast_geometry():
    """(text bytes per single-pass tile, unit starts one tile takes) of the
    loaded library (dmlc_amd_fast_geometry)."""
    t, m = ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib().dmlc_amd_fast_geometry(ctypes.byref(t), ctypes.byref(m))
    return int(t.value), int(m.value)


def make_params(fmt="libsvm", index_bits=32, value_type="f32", indexing_mode=0, label_column=-1,
                weight_column=-1, delimiter=",", tile_bytes=0, flags=0, nthread=1):
    p = Params()
    p.format = _FMT[fmt] if isinstance(fmt, str) else int(fmt)
    p.index_bits = index_bits
    p.value_type = _VT[value_type] if isinstance(value_type, str) else int(value_type)
    p.indexing_mode = indexing_mode
    p.label_column = label_column
    p.weight_column = weight_column
    p.delimiter = ord(delimiter) if isinstance(delimiter, str) else int(delimiter)
    p.tile_bytes = tile_bytes
    p.flags = flags
    p.nthread = nthread
    return p


def units_per_chunk(params):
    """ParseBlock units per chunk (FillData ranges, dmlc_amd_params.nthread)."""
    return max(int(params.nthread), 1)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("dmlc_amd: no HIP device visible")
    return torch


def _vdt(torch, vt):
    return {F32: torch.float32, I32: torch.int32, I64: torch.int64}[vt]


class DeviceParser:
    """One parser configuration bound to the current HIP device.

    parse(text, chunk_starts) takes a device uint8 tensor and a device int64
    tensor of nchunks+1 chunk boundaries and returns device tensors.

    The *_into / *_async calls with every buffer passed in can be captured into
    a graph (torch.cuda.graph) once an eager call has grown the workspaces: a
    workspace that has to grow is freed and allocated anew, and a graph
    captured earlier would keep the freed pointer.  So capture the largest
    input first, or use one parser per graph."""

    def __init__(self, fmt="libsvm", **kw):
        self.params = make_params(fmt, **kw)
        self.torch = _torch()
        self._ws = None
        self._gws = None  # gather_rows_async's workspace
        self._cws = None  # to_csc_async's
        self._qws = None  # make_cuts_async's

    def _workspace(self, nbytes, nchunks):
        need = lib().dmlc_amd_workspace_bytes(nbytes, nchunks, ctypes.byref(self.params))
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.torch.empty(need, dtype=self.torch.uint8, device="cuda")
        return self._ws, need

    def _call(self, text, chunk_starts, csr, chunk_table, result, params, stream):
        torch = self.torch
        nbytes = int(text.numel())
        nchunks = int(chunk_starts.numel()) - 1
        ws, need = self._workspace(nbytes, max(nchunks, 1))
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = lib().dmlc_amd_parse(text.data_ptr() if nbytes else None, nbytes,
                                  chunk_starts.data_ptr() if nbytes else None, nchunks,
                                  ctypes.byref(params), ctypes.byref(csr),
                                  chunk_table.data_ptr() if chunk_table is not None else None,
                                  ws.data_ptr(), ws.numel(), result.data_ptr(), s.cuda_stream)
        if rc != 0:
            msg = lib().dmlc_amd_error_string(rc).decode()
            if rc == 33:
                msg += " (%s)" % lib().dmlc_amd_last_hip_error().decode()
            raise RuntimeError("dmlc_amd_parse: %s" % msg)

    def count(self, text, chunk_starts, stream=None, result=None):
        """Size query: exact per-slot totals (device work, then a host sync).
        The per-tile counts stay in this parser's workspace for fill()."""
        torch = self.torch
        res = result if result is not None else torch.zeros(16, dtype=torch.int64, device="cuda")
        self.count_async(text, chunk_starts, res, stream=stream)
        if stream is not None:
            stream.synchronize()
        return res.cpu().numpy().view(np.uint64)

    def count_async(self, text, chunk_starts, result, out=None, stream=None):
        """Launch the count phase (count -> scan) without a host sync."""
        p = Params.from_buffer_copy(self.params)
        p.flags |= FLAG_COUNT_ONLY
        csr = Csr() if out is None else out.get("_csr") or self.csr_of(out)
        self._call(text, chunk_starts, csr, None, result, p, stream)

    def fill_async(self, text, chunk_starts, out, result, chunk_table=None, stream=None):
        """Launch the write pass over the counts of the preceding count phase."""
        p = Params.from_buffer_copy(self.params)
        p.flags |= FLAG_FILL_ONLY
        self._call(text, chunk_starts, out.get("_csr") or self.csr_of(out), chunk_table, result, p,
                   stream)

    def alloc(self, counts):
        """Allocate exact-size outputs for the given totals."""
        torch = self.torch
        wide = self.params.index_bits == 64
        it = torch.int64 if wide else torch.int32
        vt = _vdt(torch, self.params.value_type if self.params.format == CSV else F32)
        c = [int(x) for x in counts]
        out = {
            "offset": torch.empty(c[ROWS] + 1, dtype=torch.int64, device="cuda"),
            "label": torch.empty(max(c[LABEL], 1), dtype=vt, device="cuda"),
            "weight": torch.empty(max(c[WEIGHT], 1), dtype=torch.float32, device="cuda"),
            "qid": torch.empty(max(c[QID], 1), dtype=torch.int64, device="cuda"),
            "field": torch.empty(max(c[FIELD], 1), dtype=it, device="cuda"),
            "index": torch.empty(max(c[INDEX], 1), dtype=it, device="cuda"),
            "value": torch.empty(max(c[VALUE], 1), dtype=vt, device="cuda"),
            "counts": c,
        }
        return out

    def csr_of(self, out):
        csr = Csr()
        for k in ("offset", "label", "weight", "qid", "field", "index", "value"):
            setattr(csr, k, out[k].data_ptr())
        c = out["counts"]
        caps = [c[ROWS], c[INDEX], c[VALUE], c[WEIGHT], c[QID], c[LABEL], c[FIELD], 0]
        for i, v in enumerate(caps):
            csr.cap[i] = v
        return csr

    def parse_into(self, text, chunk_starts, out, result, chunk_table=None, stream=None):
        """Launch the full pipeline into preallocated outputs (no host sync)."""
        self._call(text, chunk_starts, out["_csr"] if "_csr" in out else self.csr_of(out),
                   chunk_table, result, self.params, stream)

    def parse(self, text, chunk_starts, stream=None):
        """Count, allocate, fill; returns dict of device tensors + counts/error."""
        torch = self.torch
        res = torch.zeros(16, dtype=torch.int64, device="cuda")
        counts = self.count(text, chunk_starts, stream, result=res)
        out = self.alloc(counts)
        nchunks = int(chunk_starts.numel()) - 1
        nunits = nchunks * units_per_chunk(self.params)
        out["chunk_table"] = torch.zeros(max(nunits, 1) * 8, dtype=torch.int64, device="cuda")
        self.fill_async(text, chunk_starts, out, res,
                        chunk_table=out["chunk_table"] if nchunks > 0 else None, stream=stream)
        r = res.cpu().numpy().view(np.uint64)
        out["error"] = int(r[8])
        out["path"] = int(r[9])
        out["result_counts"] = [int(x) for x in r[:8]]
        out["max_index"], out["max_field"] = int(r[10]), int(r[11])
        out["result"] = res  # the device result block (to_dense reads its counts)
        return out

    # ---- dense row batches (dmlc_amd_to_dense)
    def _value_type(self):
        return self.params.value_type if self.params.format == CSV else F32

    def to_dense_async(self, out, result, dense, *, ncol, row_begin=0, max_rows=None, fill=float("nan"),
                       fill_bits=None, status=None, stream=None):
        """Launch the CSR -> dense pass behind the parse that fills `result`
        (same stream, no host sync): rows [row_begin, row_begin + max_rows) of
        the parsed batch `out` into `dense`, a 2-D device tensor of the value
        dtype with ncol columns (a strided view is fine: ld = dense.stride(0)).
        max_rows defaults to dense.shape[0]; rows the parse did not produce
        stay unwritten.  `fill` goes into cells without an entry, by value or
        as an explicit bit pattern `fill_bits`.  Returns the device status
        tensor (int64[4]: rows written, entries dropped, first dropped
        position, DENSE_FLAG_* bits)."""
        torch = self.torch
        vt = self._value_type()
        if dense.dim() != 2 or int(dense.shape[1]) != int(ncol) or dense.dtype != _vdt(torch, vt):
            raise ValueError("dense must be a 2-D %s tensor with ncol = %d columns" % (_vdt(torch, vt), ncol))
        if int(ncol) > 1 and dense.stride(1) != 1:
            raise ValueError("dense rows must be contiguous (stride(1) == 1)")
        nrow = int(dense.shape[0])
        if max_rows is None:
            max_rows = nrow
        if max_rows > nrow:
            raise ValueError("max_rows = %d exceeds the %d rows of dense" % (max_rows, nrow))
        if status is None:
            status = torch.empty(4, dtype=torch.int64, device=dense.device)
        p = DenseParams()
        p.index_bits = self.params.index_bits
        p.value_type = vt
        p.row_begin, p.max_rows, p.ncol = int(row_begin), int(max_rows), int(ncol)
        p.ld = max(int(dense.stride(0)), int(ncol)) if nrow > 1 else int(ncol)
        p.fill_bits = int(fill_bits) if fill_bits is not None else fill_bits_of(fill, vt)
        csr = out.get("_csr") or self.csr_of(out)
        s = stream if stream is not None else torch.cuda.current_stream()
        # (an empty tensor has no storage: max_rows == 0 only sets the status, any non-null pointer does)
        rc = lib().dmlc_amd_to_dense(ctypes.byref(csr), result.data_ptr(), ctypes.byref(p),
                                     dense.data_ptr() if nrow else status.data_ptr(), status.data_ptr(),
                                     s.cuda_stream)
        if rc != 0:
            msg = lib().dmlc_amd_error_string(rc).decode()
            if rc == 33:
                msg += " (%s)" % lib().dmlc_amd_last_hip_error().decode()
            raise RuntimeError("dmlc_amd_to_dense: %s" % msg)
        return status

    def to_dense(self, out, ncol=None, fill=float("nan"), row_begin=0, max_rows=None, fill_bits=None):
        """Dense rows of a batch returned by parse(): (tensor, status) after a
        sync, status as uint64[4].  ncol=None means max_index + 1 (the NumCol
        of the reference's BasicRowIter), which needs a parser made with
        flags=FLAG_MAX_INDEX."""
        torch = self.torch
        if ncol is None:
            if not self.params.flags & FLAG_MAX_INDEX:
                raise ValueError("ncol=None needs a parse made with FLAG_MAX_INDEX (result.max_index)")
            ncol = int(out["max_index"]) + 1
        rows = int(out["counts"][ROWS])
        if max_rows is None:
            max_rows = max(rows - int(row_begin), 0)
        dense = torch.empty((int(max_rows), int(ncol)), dtype=_vdt(torch, self._value_type()), device="cuda")
        status = self.to_dense_async(out, out["result"], dense, ncol=ncol, row_begin=row_begin,
                                     max_rows=max_rows, fill=fill, fill_bits=fill_bits)
        return dense, status.cpu().numpy().view(np.uint64)

    def parse_dense(self, text, chunk_starts, ncol, fill=float("nan"), fill_bits=None, stream=None):
        """Text -> dense rows: count, allocate, then the write pass and the
        dense pass on one stream with no host sync between the two.  Returns
        parse()'s dict with "dense" (rows x ncol) and "dense_status"."""
        torch = self.torch
        res = torch.zeros(16, dtype=torch.int64, device="cuda")
        counts = self.count(text, chunk_starts, stream, result=res)
        out = self.alloc(counts)
        nchunks = int(chunk_starts.numel()) - 1
        out["chunk_table"] = torch.zeros(max(nchunks * units_per_chunk(self.params), 1) * 8, dtype=torch.int64,
                                         device="cuda")
        dense = torch.empty((int(counts[ROWS]), int(ncol)), dtype=_vdt(torch, self._value_type()), device="cuda")
        self.fill_async(text, chunk_starts, out, res, chunk_table=out["chunk_table"] if nchunks > 0 else None,
                        stream=stream)
        status = self.to_dense_async(out, res, dense, ncol=ncol, fill=fill, fill_bits=fill_bits, stream=stream)
        if stream is not None:
            stream.synchronize()
        r = res.cpu().numpy().view(np.uint64)
        out["error"], out["path"] = int(r[8]), int(r[9])
        out["result_counts"] = [int(x) for x in r[:8]]
        out["max_index"], out["max_field"] = int(r[10]), int(r[11])
        out["result"] = res
        out["dense"] = dense
        out["dense_status"] = status.cpu().numpy().view(np.uint64)
        return out

    # ---- quantised dense row batches (dmlc_amd_to_bins)
    def to_bins_async(self, out, result, bins, cut_ptr, cut_value, *, ncol, row_begin=0, max_rows=None, missing=None,
                      global_ids=False, status=None, stream=None):
        """Launch the CSR -> bin codes pass behind whatever fills `result`
        (same stream, no host sync): rows [row_begin, row_begin + max_rows) of
        the batch `out` into `bins`, a 2-D device uint8 / int16 / int32 tensor
        with ncol columns whose dtype chooses the code width (a strided view
        is fine: ld = bins.stride(0)).  cut_ptr is a device int32 tensor of
        ncol + 1 words (read as unsigned), cut_value a device float32 tensor:
        column c's cuts are cut_value[cut_ptr[c] : cut_ptr[c + 1]], ascending.
        A cell's code is min(#{cuts <= v}, cuts - 1), plus cut_ptr[c] with
        global_ids; `missing` (default: the all-ones code of that width) goes
        into cells without an entry, with a NaN or without cuts.  max_rows
        defaults to bins.shape[0]; rows the parse did not produce stay
        unwritten.  Returns the device status tensor (int64[8]: rows written,
        entries dropped, first dropped position, DENSE_FLAG_* | BINS_FLAG_*
        bits, NaN cells, unbinned cells, 0, 0)."""
        torch = self.torch
        if self._value_type() != F32:
            raise ValueError("to_bins takes float values only")
        widths = {torch.uint8: 1, torch.int16: 2, torch.int32: 4}
        if bins.dim() != 2 or int(bins.shape[1]) != int(ncol) or bins.dtype not in widths:
            raise ValueError("bins must be a 2-D uint8, int16 or int32 tensor with ncol = %d columns" % ncol)
        if int(ncol) > 1 and bins.stride(1) != 1:
            raise ValueError("bins rows must be contiguous (stride(1) == 1)")
        if cut_ptr.dtype != torch.int32 or cut_ptr.dim() != 1 or int(cut_ptr.numel()) < int(ncol) + 1 \
                or not cut_ptr.is_contiguous():
            raise ValueError("cut_ptr must be a contiguous int32 tensor of ncol + 1 = %d words" % (int(ncol) + 1))
        if cut_value.dtype != torch.float32 or cut_value.dim() != 1 or not cut_value.is_contiguous():
            raise ValueError("cut_value must be a contiguous 1-D float32 tensor")
        nrow = int(bins.shape[0])
        if max_rows is None:
            max_rows = nrow
        if max_rows > nrow:
            raise ValueError("max_rows = %d exceeds the %d rows of bins" % (max_rows, nrow))
        if nrow > 1 and int(bins.stride(0)) < int(ncol):
            raise ValueError("bins rows overlap (stride(0) = %d < ncol = %d)" % (bins.stride(0), ncol))
        if status is None:
            status = torch.empty(8, dtype=torch.int64, device=bins.device)
        p = BinsParams()
        p.index_bits = self.params.index_bits
        p.value_type = F32
        p.code_bytes = widths[bins.dtype]
        p.missing_code = (1 << (8 * p.code_bytes)) - 1 if missing is None else int(missing) & 0xFFFFFFFF
        p.row_begin, p.max_rows, p.ncol = int(row_begin), int(max_rows), int(ncol)
        p.ld = int(bins.stride(0)) if nrow > 1 else int(ncol)
        p.flags = BINS_GLOBAL if global_ids else 0
        c = Cuts()
        n_cuts = int(cut_value.numel())
        c.cut_ptr, c.cut_value, c.n_cuts = cut_ptr.data_ptr(), cut_value.data_ptr() if n_cuts else None, n_cuts
        csr = out.get("_csr") or self.csr_of(out)
        s = stream if stream is not None else torch.cuda.current_stream()
        # (an empty tensor has no storage: max_rows == 0 only sets the status, any non-null pointer does)
        rc = lib().dmlc_amd_to_bins(ctypes.byref(csr), result.data_ptr(), ctypes.byref(c), ctypes.byref(p),
                                    bins.data_ptr() if nrow else status.data_ptr(), status.data_ptr(),
                                    s.cuda_stream)
        if rc != 0:
            msg = lib().dmlc_amd_error_string(rc).decode()
            if rc == 33:
                msg += " (%s)" % lib().dmlc_amd_last_hip_error().decode()
            raise RuntimeError("dmlc_amd_to_bins: %s" % msg)
        return status

    def to_bins(self, out, cut_ptr, cut_value, ncol=None, dtype=None, row_begin=0, max_rows=None, missing=None,
                global_ids=False):
        """Bin codes of a batch returned by parse() or gather_rows(): (tensor,
        status) after a sync, status as uint64[8].  dtype (default
        torch.uint8) chooses the code width.  ncol=None means
        len(cut_ptr) - 1."""
        torch = self.torch
        if ncol is None:
            ncol = int(cut_ptr.numel()) - 1
        rows = int(out["counts"][ROWS])
        if max_rows is None:
            max_rows = max(rows - int(row_begin), 0)
        bins = torch.empty((int(max_rows), int(ncol)), dtype=dtype or torch.uint8, device="cuda")
        status = self.to_bins_async(out, out["result"], bins, cut_ptr, cut_value, ncol=ncol, row_begin=row_begin,
                                    max_rows=max_rows, missing=missing, global_ids=global_ids)
        return bins, status.cpu().numpy().view(np.uint64)

    def parse_bins(self, text, chunk_starts, cut_ptr, cut_value, ncol, dtype=None, missing=None, global_ids=False,
                   stream=None):
        """Text -> bin codes: count, allocate, then the write pass and the
        bins pass on one stream with no host sync between the two.  Returns
        parse()'s dict with "bins" (rows x ncol) and "bins_status"."""
        torch = self.torch
        res = torch.zeros(16, dtype=torch.int64, device="cuda")
        counts = self.count(text, chunk_starts, stream, result=res)
        out = self.alloc(counts)
        nchunks = int(chunk_starts.numel()) - 1
        out["chunk_table"] = torch.zeros(max(nchunks * units_per_chunk(self.params), 1) * 8, dtype=torch.int64,
                                         device="cuda")
        bins = torch.empty((int(counts[ROWS]), int(ncol)), dtype=dtype or torch.uint8, device="cuda")
        self.fill_async(text, chunk_starts, out, res, chunk_table=out["chunk_table"] if nchunks > 0 else None,
                        stream=stream)
        status = self.to_bins_async(out, res, bins, cut_ptr, cut_value, ncol=ncol, missing=missing,
                                    global_ids=global_ids, stream=stream)
        if stream is not None:
            stream.synchronize()
        r = res.cpu().numpy().view(np.uint64)
        out["error"], out["path"] = int(r[8]), int(r[9])
        out["result_counts"] = [int(x) for x in r[:8]]
        out["max_index"], out["max_field"] = int(r[10]), int(r[11])
        out["result"] = res
        out["bins"] = bins
        out["bins_status"] = status.cpu().numpy().view(np.uint64)
        return out

    # ---- per-column quantile cut points (dmlc_amd_make_cuts)
    def make_cuts_async(self, out, result, cut_ptr, cut_value, status=None, *, ncol, max_bin=256, row_begin=0,
                        max_rows=None, stream=None):
        """Launch the quantile sketch behind whatever fills `result` (same
        stream, no host sync): for every column below ncol the deduplicated
        exact rank quantiles (at most max_bin cuts, the last just above the
        column's maximum) of the entries in rows [row_begin, row_begin +
        max_rows) of the batch `out`.  cut_ptr is a device int32 tensor of
        ncol + 1 words (written as unsigned), cut_value a device float32
        tensor whose length is the capacity (ncol * max_bin always suffices);
        both go straight into to_bins_async.  Returns the device status tensor
        (int64[8]: entries kept, entries dropped, first dropped position,
        CSC_FLAG_* bits, NaN samples, cuts, columns without cuts, 0)."""
        torch = self.torch
        if self._value_type() != F32:
            raise ValueError("make_cuts takes float values only")
        if cut_ptr.dtype != torch.int32 or cut_ptr.dim() != 1 or int(cut_ptr.numel()) < int(ncol) + 1 \
                or not cut_ptr.is_contiguous():
            raise ValueError("cut_ptr must be a contiguous int32 tensor of ncol + 1 = %d words" % (int(ncol) + 1))
        if cut_value.dtype != torch.float32 or cut_value.dim() != 1 or not cut_value.is_contiguous():
            raise ValueError("cut_value must be a contiguous 1-D float32 tensor")
        if status is None:
            status = torch.empty(8, dtype=torch.int64, device=cut_ptr.device)
        p = MakeCutsParams()
        p.index_bits = self.params.index_bits
        p.value_type = F32
        p.row_begin = int(row_begin)
        p.max_rows = (1 << 64) - 1 if max_rows is None else int(max_rows)
        p.ncol = int(ncol)
        p.max_bin = int(max_bin)
        src = out.get("_csr") or self.csr_of(out)
        m = int(src.cap[INDEX])
        p.max_entries = m
        need = lib().dmlc_amd_make_cuts_workspace_bytes(m, int(ncol), ctypes.byref(p))
        if need == 0:
            raise ValueError("dmlc_amd_make_cuts: bad ncol = %d or max_bin = %d (ncol * max_bin < 2^32), or a batch "
                             "of 2^32 - 1 or more entries" % (int(ncol), int(max_bin)))
        if self._qws is None or self._qws.numel() < need:
            self._qws = torch.empty(need, dtype=torch.uint8, device="cuda")
        c = CutsOut()
        cap = int(cut_value.numel())
        c.cut_ptr, c.cut_value, c.cap = cut_ptr.data_ptr(), cut_value.data_ptr() if cap else None, cap
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = lib().dmlc_amd_make_cuts(ctypes.byref(src), result.data_ptr(), ctypes.byref(p), ctypes.byref(c),
                                      status.data_ptr(), self._qws.data_ptr(), self._qws.numel(), s.cuda_stream)
        if rc != 0:
            msg = lib().dmlc_amd_error_string(rc).decode()
            if rc == 33:
                msg += " (%s)" % lib().dmlc_amd_last_hip_error().decode()
            raise RuntimeError("dmlc_amd_make_cuts: %s" % msg)
        return status

    def make_cuts(self, out, ncol=None, max_bin=256, row_begin=0, max_rows=None):
        """Cut points of a batch returned by parse() or gather_rows():
        (cut_ptr int32[ncol + 1], cut_value float32[N_CUTS], status uint64[8])
        after a sync.  ncol=None means max_index + 1, which needs a parser made
        with flags=FLAG_MAX_INDEX.  Raises on a failed parse, a bad value
        count, a capacity overflow or a truncated window (flag bits 0, 1, 3,
        4)."""
        torch = self.torch
        if ncol is None:
            if not self.params.flags & FLAG_MAX_INDEX:
                raise ValueError("ncol=None needs a parse made with FLAG_MAX_INDEX (result.max_index)")
            ncol = int(out["max_index"]) + 1
        # a column holds at most min(max_bin, its samples) cuts
        cap = min(int(ncol) * int(max_bin), int(out["counts"][INDEX]))
        cut_ptr = torch.empty(int(ncol) + 1, dtype=torch.int32, device="cuda")
        cut_value = torch.empty(cap, dtype=torch.float32, device="cuda")
        status = self.make_cuts_async(out, out["result"], cut_ptr, cut_value, ncol=ncol, max_bin=max_bin,
                                      row_begin=row_begin, max_rows=max_rows).cpu().numpy().view(np.uint64)
        bad = int(status[CSC_FLAGS]) & (CSC_FLAG_ERROR | CSC_FLAG_VALUE_COUNT | CSC_FLAG_CAPACITY | CSC_FLAG_MAX_ENTRIES)
        if bad:
            raise RuntimeError("dmlc_amd_make_cuts: status flags %#x" % int(status[CSC_FLAGS]))
        return cut_ptr, cut_value[:int(status[CUTS_N_CUTS])], status

    # ---- row gather: shuffle / select rows of a parsed batch (dmlc_amd_gather_rows)
    def gather_rows_async(self, out, result, ids, dst=None, dst_result=None, status=None, stream=None):
        """Launch the row gather behind whatever fills `result` (same stream,
        no host sync): rows ids[0 .. n) of the batch `out`, in that order, as
        a new compact CSR.  `ids` is a device int32 or int64 tensor (read as
        unsigned; an id at or past the batch's rows gives an empty row and is
        counted).  `dst` is an alloc()-style dict sized by the caller; the
        default holds len(ids) rows and as many entries as the whole source
        (out["counts"]), which is enough when no id repeats.  Returns (dst,
        dst_result, status): the device result block (dmlc_amd_result layout:
        exact counts, error) and the device status tensor (int64[4]: rows
        written, bad ids, first bad position, GATHER_FLAG_* bits).  dst and
        dst_result go straight into to_dense_async or another gather."""
        torch = self.torch
        if ids.dim() != 1 or ids.dtype not in (torch.int32, torch.int64) or not ids.is_contiguous():
            raise ValueError("ids must be a contiguous 1-D device int32 or int64 tensor")
        n = int(ids.numel())
        if dst is None:
            c = list(out["counts"]) + [0] * (8 - len(out["counts"]))
            for slot in (ROWS, WEIGHT, QID, LABEL):
                c[slot] = n
            c[VALUE] = c[FIELD] = c[INDEX]  # (which per-entry arrays exist is known on the device)
            dst = self.alloc(c)
        if dst_result is None:
            dst_result = torch.empty(16, dtype=torch.int64, device=ids.device)
        if status is None:
            status = torch.empty(4, dtype=torch.int64, device=ids.device)
        need = lib().dmlc_amd_gather_workspace_bytes(n)
        if self._gws is None or self._gws.numel() < need:
            self._gws = torch.empty(need, dtype=torch.uint8, device="cuda")
        p = GatherParams()
        p.index_bits = self.params.index_bits
        p.value_type = p.label_type = self._value_type()
        p.id_bits = 64 if ids.dtype == torch.int64 else 32
        p.flags = self.params.flags & FLAG_MAX_INDEX
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = lib().dmlc_amd_gather_rows(ctypes.byref(out.get("_csr") or self.csr_of(out)), result.data_ptr(),
                                        ids.data_ptr() if n else None, n, ctypes.byref(p),
                                        ctypes.byref(dst.get("_csr") or self.csr_of(dst)), dst_result.data_ptr(),
                                        status.data_ptr(), self._gws.data_ptr(), self._gws.numel(), s.cuda_stream)
        if rc != 0:
            msg = lib().dmlc_amd_error_string(rc).decode()
            if rc == 33:
                msg += " (%s)" % lib().dmlc_amd_last_hip_error().decode()
            raise RuntimeError("dmlc_amd_gather_rows: %s" % msg)
        return dst, dst_result, status

    def gather_rows(self, out, ids):
        """Rows `ids` of a batch returned by parse() (or by gather_rows): sizes
        the new batch exactly, syncs, and returns a dict shaped like parse()'s
        (the arrays, "counts", "result", "error", "max_index", ...) with
        "gather_status" (uint64[4]) added; to_host, to_dense and gather_rows
        take it."""
        torch = self.torch
        n = int(ids.numel())
        # the exact entry count: the selected rows' lengths (bad ids: none)
        rows = int(out["counts"][ROWS])
        if n and rows:
            r = ids.long()
            ok = (r >= 0) & (r < rows)
            r = torch.where(ok, r, torch.zeros_like(r))
            off = out["offset"]
            nnz = int(torch.where(ok, off[r + 1] - off[r], torch.zeros_like(r)).sum().item())
        else:
            nnz = 0
        sc = out["counts"]
        c = [0] * 8
        c[ROWS], c[INDEX] = n, nnz
        c[VALUE] = nnz if sc[VALUE] else 0
        c[FIELD] = nnz if sc[FIELD] else 0
        for slot in (WEIGHT, QID, LABEL):
            c[slot] = n if sc[slot] and sc[slot] == sc[ROWS] else 0
        dst = self.alloc(c)
        _, res, status = self.gather_rows_async(out, out["result"], ids, dst=dst)
        r = res.cpu().numpy().view(np.uint64)
        dst["counts"] = [int(x) for x in r[:8]]
        dst["result_counts"] = list(dst["counts"])
        dst["error"], dst["path"] = int(r[8]), int(r[9])
        dst["max_index"], dst["max_field"] = int(r[10]), int(r[11])
        dst["result"] = res
        dst["gather_status"] = status.cpu().numpy().view(np.uint64)
        return dst

    # ---- the column view: CSC transpose of a parsed batch (dmlc_amd_to_csc)
    def to_csc_async(self, out, result, csc, status=None, *, ncol, row_begin=0, max_rows=None, stream=None):
        """Launch the CSC transpose behind whatever fills `result` (same
        stream, no host sync): the entries of rows [row_begin, row_begin +
        max_rows) of the batch `out` by column, each column in ascending
        source position.  `csc` is a dict of device tensors: "col_offset"
        (int64[ncol + 1]), "row" (int32[cap]), and optionally "value" (the
        value dtype, [cap]) and "pos" (int64[cap], each entry's source
        position); cap is the length of "row".  max_rows defaults to every row
        from row_begin on.  Returns the device status tensor (int64[4]:
        entries kept, entries dropped, first dropped position, CSC_FLAG_*
        bits)."""
        torch = self.torch
        vt = self._value_type()
        co, row, val, pos = csc["col_offset"], csc["row"], csc.get("value"), csc.get("pos")
        if co.dtype != torch.int64 or int(co.numel()) < int(ncol) + 1 or not co.is_contiguous():
            raise ValueError("col_offset must be a contiguous int64 tensor of ncol + 1 = %d words" % (int(ncol) + 1))
        if row.dtype != torch.int32 or not row.is_contiguous():
            raise ValueError("row must be a contiguous int32 tensor")
        cap = int(row.numel())
        if val is not None and (val.dtype != _vdt(torch, vt) or int(val.numel()) < cap or not val.is_contiguous()):
            raise ValueError("value must be a contiguous %s tensor of at least len(row) elements" % _vdt(torch, vt))
        if pos is not None and (pos.dtype != torch.int64 or int(pos.numel()) < cap or not pos.is_contiguous()):
            raise ValueError("pos must be a contiguous int64 tensor of at least len(row) elements")
        if status is None:
            status = torch.empty(4, dtype=torch.int64, device=co.device)
        p = CscParams()
        p.index_bits = self.params.index_bits
        p.value_type = vt
        p.row_begin = int(row_begin)
        p.max_rows = (1 << 64) - 1 if max_rows is None else int(max_rows)
        p.ncol = int(ncol)
        src = out.get("_csr") or self.csr_of(out)
        m = int(src.cap[INDEX])
        p.max_entries = m
        need = lib().dmlc_amd_csc_workspace_bytes(m, int(ncol), ctypes.byref(p))
        if need == 0:
            raise ValueError("dmlc_amd_to_csc: bad ncol = %d or a batch of 2^32 - 1 or more entries" % int(ncol))
        if self._cws is None or self._cws.numel() < need:
            self._cws = torch.empty(need, dtype=torch.uint8, device="cuda")
        c = Csc()
        c.col_offset, c.row = co.data_ptr(), row.data_ptr() if cap else status.data_ptr()
        c.value = val.data_ptr() if val is not None and cap else None
        c.pos = pos.data_ptr() if pos is not None and cap else None
        c.cap = cap
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = lib().dmlc_amd_to_csc(ctypes.byref(src), result.data_ptr(), ctypes.byref(p), ctypes.byref(c),
                                   status.data_ptr(), self._cws.data_ptr(), self._cws.numel(), s.cuda_stream)
        if rc != 0:
            msg = lib().dmlc_amd_error_string(rc).decode()
            if rc == 33:
                msg += " (%s)" % lib().dmlc_amd_last_hip_error().decode()
            raise RuntimeError("dmlc_amd_to_csc: %s" % msg)
        return status

    def to_csc(self, out, ncol=None, want_pos=False):
        """The column view of a batch returned by parse() or gather_rows():
        a dict with "col_offset" (int64[ncol + 1]), "row" (int32), "value"
        (None for a batch without values) and, with want_pos, "pos" (int64:
        each entry's position in the batch's arrays, e.g. out["field"][pos]),
        trimmed to the kept entries after a sync; "status" is uint64[4].
        ncol=None means max_index + 1, which needs a parser made with
        flags=FLAG_MAX_INDEX."""
        torch = self.torch
        if ncol is None:
            if not self.params.flags & FLAG_MAX_INDEX:
                raise ValueError("ncol=None needs a parse made with FLAG_MAX_INDEX (result.max_index)")
            ncol = int(out["max_index"]) + 1
        c = out["counts"]
        cap = int(c[INDEX])
        csc = {"col_offset": torch.empty(int(ncol) + 1, dtype=torch.int64, device="cuda"),
               "row": torch.empty(cap, dtype=torch.int32, device="cuda")}
        if c[VALUE]:
            csc["value"] = torch.empty(cap, dtype=_vdt(torch, self._value_type()), device="cuda")
        if want_pos:
            csc["pos"] = torch.empty(cap, dtype=torch.int64, device="cuda")
        status = self.to_csc_async(out, out["result"], csc, ncol=ncol).cpu().numpy().view(np.uint64)
        kept = min(int(status[CSC_KEPT]), cap)
        res = {"col_offset": csc["col_offset"], "row": csc["row"][:kept],
               "value": csc["value"][:kept] if "value" in csc else None, "status": status, "ncol": int(ncol)}
        if want_pos:
            res["pos"] = csc["pos"][:kept]
        return res

    def shuffle(self, out, generator=None):
        """The batch with its rows in a fresh random order (torch.randperm on
        the device): (batch, permutation); batch row i is out's row perm[i]."""
        torch = self.torch
        perm = torch.randperm(int(out["counts"][ROWS]), device="cuda", generator=generator)
        return self.gather_rows(out, perm), perm


def build_id():
    """SHA-256 prefix of the sources the loaded library was built from."""
    L = lib()
    return L.dmlc_amd_build_id().decode() if hasattr(L, "dmlc_amd_build_id") else "unknown"


def error_code(err):
    return int(err) & 0xFFFF


def error_pos(err):
    return int(err) >> 16


def to_host(out, index_bits=32, value_type=F32):
    """Copy parse outputs to numpy with the reference's dtypes."""
    c = out["counts"]
    it = np.uint32 if index_bits == 32 else np.uint64
    vt = {F32: np.float32, I32: np.int32, I64: np.int64}[value_type]
    h = {
        "offset": out["offset"][: c[ROWS] + 1].cpu().numpy().view(np.uint64),
        "label": out["label"][: c[LABEL]].cpu().numpy().view(vt),
        "weight": out["weight"][: c[WEIGHT]].cpu().numpy().view(np.float32),
        "qid": out["qid"][: c[QID]].cpu().numpy().view(np.uint64),
        "field": out["field"][: c[FIELD]].cpu().numpy().view(it),
        "index": out["index"][: c[INDEX]].cpu().numpy().view(it),
        "value": out["value"][: c[VALUE]].cpu().numpy().view(vt),
    }
    if "chunk_table" in out:
        h["chunk_table"] = out["chunk_table"].cpu().numpy().view(np.uint64).reshape(-1, 8)
    return h


def parse_bytes(data, chunk_offsets=None, fmt="libsvm", exact=False, **kw):
    """Convenience: host bytes -> device -> parse -> host numpy dict."""
    torch = _torch()
    raw = data.encode("latin-1") if isinstance(data, str) else bytes(data)
    if chunk_offsets is None:
        chunk_offsets = [0, len(raw)] if raw else [0]
    text = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda() if raw else \
        torch.empty(0, dtype=torch.uint8, device="cuda")
    cs = torch.tensor(np.asarray(chunk_offsets, dtype=np.int64), device="cuda")
    if exact:
        kw["flags"] = kw.get("flags", 0) | FLAG_EXACT
    p = DeviceParser(fmt, **kw)
    out = p.parse(text, cs)
    h = to_host(out, p.params.index_bits,
                p.params.value_type if p.params.format == CSV else F32)
    h["error"] = out["error"]
    h["path"] = "exact" if out["path"] else "fast"
    h["counts"] = out["counts"]
    h["units_per_chunk"] = units_per_chunk(p.params)
    return h


def strtof_batch(strings):
    """Device dmlc::strtof over a list of byte strings -> (f32 values, consumed, nan_err)."""
    torch = _torch()
    raws = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in strings]
    offs = np.zeros(len(raws) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(r) for r in raws])
    blob = b"".join(raws) or b"\0"
    text = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_off = torch.tensor(offs, device="cuda")
    n = len(raws)
    out = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
    used = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    bad = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    rc = lib().dmlc_amd_strtof_batch(text.data_ptr(), d_off.data_ptr(), n, out.data_ptr(),
                                     used.data_ptr(), bad.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError("dmlc_amd_strtof_batch failed")
    torch.cuda.synchronize()
    return out[:n].cpu().numpy(), used[:n].cpu().numpy(), bad[:n].cpu().numpy()


def chunk_check(h, fmt, nchunks, total_counts):
    """Per-unit consistency CHECKs of the reference, applied to GPU output
    (nchunks: table rows, i.e. chunks x units per chunk).

    The reference raises these from RowBlockContainer::GetBlock (row_block.h:
    174-178) and, for CSV, from ParseBlock itself (csv_parser.h:147-148); libfm
    adds field == index (libfm_parser.h:127).  Returns the first failing chunk
    index or -1."""
    f = _FMT[fmt] if isinstance(fmt, str) else fmt
    tab = h["chunk_table"][:nchunks].astype(np.int64)
    ends = np.vstack([tab[1:], np.asarray(total_counts[:8], dtype=np.int64)[None, :]])
    per = ends - tab
    for c in range(nchunks):
        rows, idx, val, w, lab, fld = (per[c, ROWS], per[c, INDEX], per[c, VALUE], per[c, WEIGHT],
                                       per[c, LABEL], per[c, FIELD])
        if f == CSV:
            if lab != 0 and lab != rows:
                return c
            if w != 0 and w != rows:
                return c
        if f == LIBFM and fld != idx:
            return c
        if rows and not (val == 0 or val == idx):
            return c
    return -1


def text_chunk_starts(text, chunk_bytes=8 << 20):
    """Chunk boundaries an InputSplit ("text", one part) would hand over for
    this buffer: each chunk ends just after the last '\\n' / '\\r' inside its
    `chunk_bytes` read buffer (LineSplitter::FindLastRecordBegin,
    src/io/line_split.cc:37-45; kBufferSize, src/io/input_split_base.h:39); a
    record longer than the buffer grows it until one fits
    (input_split_base.cc:272-291).  Returns int64 [nchunks + 1] offsets."""
    a = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    n = int(a.size)
    if n == 0:
        return np.zeros(1, dtype=np.int64)
    nl = np.flatnonzero((a == 10) | (a == 13)) + 1  # candidate chunk ends (record begins)
    starts = [0]
    s = 0
    while s < n:
        lim = s + chunk_bytes
        if lim >= n:
            starts.append(n)
            break
        while True:
            # last newline at p with s < p < lim; the record begins at p + 1
            j = int(np.searchsorted(nl, lim, side="right")) - 1
            if j >= 0 and int(nl[j]) - 1 > s:
                e = int(nl[j])
                break
            lim = s + (lim - s) * 2  # record longer than the buffer: grow
            if lim >= n:
                e = n
                break
        starts.append(e)
        s = e
    return np.asarray(starts, dtype=np.int64)
