"""ctypes mirror of include/pandepth_amd.h (one method per entry point, same names/arguments).

Plumbing only: numpy arrays in, numpy arrays out, raw device pointers accepted for HBM-resident
batches (e.g. torch tensors' data_ptr()).  Every failure of the C-ABI raises PdError with the
library's own message; there is no alternative code path.
"""
import ctypes
import os

import numpy as np

PD_PUSH_DEFAULT = 0
PD_PUSH_SORTED = 1
PD_PUSH_MORE = 2


def PD_PUSH_DISORDER(cells):
    return ((int(cells) + 255) // 256) << 8

PD_TILE = 8192
PD_UNIT_GUESS = 1
PD_DECODE_COMPACT = 1
PD_DECODE_DELETIONS = 2
PD_DECODE_FRAGMENTS = 4
PD_DECODE_RECORD_STATS = 8
PD_DECODE_ROW_COUNTS = 16
PD_DECODE_ALN_STATS = 32
PD_ALNSTAT_WORDS = 8 + 20 + 2 * 257 + 101 + 4 * 8192   # pd_decode_aln_stats: the sums (include/pandepth_amd.h)
PD_ROWCOUNT_WORDS = 6                    # pd_decode_row_counts: the words of a bin (include/pandepth_amd.h)
PD_RECSTAT_FIXED = 275                   # pd_decode_record_stats: the sums before the insert bins (include/pandepth_amd.h)
PD_NONE = 0xFFFFFFFFFFFFFFFF                     # pd_decode_result::first_start / next_start: no such record


# ---- the decode session's structs (include/pandepth_amd.h; tests/test_capi_layout.py holds them to the header's sizeof / offsetof) ----
class pd_bgzf_block(ctypes.Structure):
    _fields_ = [("in_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("in_len", ctypes.c_uint32), ("out_len", ctypes.c_uint32)]


class pd_decode_cfg(ctypes.Structure):
    _fields_ = [("flag_mask", ctypes.c_uint32), ("min_mapq", ctypes.c_int32), ("contig_on", ctypes.c_void_p), ("span_off", ctypes.c_void_p),
                ("spans", ctypes.c_void_p), ("sorted", ctypes.c_int32), ("bytes_hint", ctypes.c_uint64), ("batch_bytes", ctypes.c_uint64),
                ("batches_in_flight", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_batches", ctypes.c_uint64)]


class pd_decode_unit(ctypes.Structure):
    _fields_ = [("start", ctypes.c_uint64), ("stop", ctypes.c_uint64), ("avail", ctypes.c_uint64), ("first_block", ctypes.c_uint32),
                ("n_blocks", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class pd_decode_batch(ctypes.Structure):
    _fields_ = [("host_buf", ctypes.c_void_p), ("n_bytes", ctypes.c_size_t), ("blocks", ctypes.POINTER(pd_bgzf_block)), ("n_blocks", ctypes.c_uint32),
                ("pad", ctypes.c_uint32), ("inflated_bytes", ctypes.c_uint64), ("units", ctypes.POINTER(pd_decode_unit)), ("n_units", ctypes.c_uint32),
                ("pad2", ctypes.c_uint32), ("order", ctypes.c_uint64)]


class pd_decode_result(ctypes.Structure):
    _fields_ = [("n_reads", ctypes.c_uint64), ("n_first", ctypes.c_uint64), ("n_other", ctypes.c_uint64), ("first_start", ctypes.c_uint64),
                ("next_start", ctypes.c_uint64), ("ms_h2d", ctypes.c_double), ("ms_inflate", ctypes.c_double), ("ms_walk", ctypes.c_double),
                ("ms_emit", ctypes.c_double), ("first_key", ctypes.c_uint64), ("last_key", ctypes.c_uint64), ("unsorted", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]


DECODE_STRUCTS = [pd_bgzf_block, pd_decode_cfg, pd_decode_unit, pd_decode_batch, pd_decode_result]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

IV_DTYPE = np.dtype([("tid", "<i4"), ("beg", "<i4"), ("end", "<i4")])


class PdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pandepth_amd error %d: %s" % (code, msg))
        self.code = code


def lib_path():
    # (PANDEPTH_AMD_LIB: a tuning build of the library, tools/ubench only)
    return os.environ.get("PANDEPTH_AMD_LIB") or os.path.join(_HERE, "libpandepth_amd.so")


def load():
    """Load libpandepth_amd.so (built in-tree by `make -C pandepth_amd` / __graft_entry__.build)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise PdError(-2, "libpandepth_amd.so is not built (run `make -C pandepth_amd`); "
                          "there is no CPU fallback")
    L = ctypes.CDLL(p)
    P, I, U, U64, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint64, ctypes.c_size_t
    sig = {
        "pd_abi_version": (I, []),
        "pd_create": (I, [I, ctypes.c_int32, P, ctypes.POINTER(P)]),
        "pd_destroy": (I, [P]),
        "pd_strerror": (ctypes.c_char_p, [P]),
        "pd_reset": (I, [P]),
        "pd_push_intervals": (I, [P, P, SZ, U]),
        "pd_push_intervals_device": (I, [P, P, SZ, U]),
        "pd_runs_create": (I, [P, P, SZ, P, SZ, ctypes.POINTER(P)]),
        "pd_runs_destroy": (I, [P]),
        "pd_push_runs": (I, [P, P, U]),
        "pd_stage_acquire": (I, [P, ctypes.POINTER(P), ctypes.POINTER(SZ)]),
        "pd_stage_submit": (I, [P, P, SZ, U]),
        "pd_set_param": (I, [P, ctypes.c_char_p, U64]),
        "pd_keep_deferred": (I, [P, I]),
        "pd_scan": (I, [P, U]),
        "pd_reduce_intervals": (I, [P, P, SZ, ctypes.c_uint32, P, P]),
        "pd_window_layout": (I, [P, ctypes.c_uint32, P]),
        "pd_scan_reduce_windows": (I, [P, ctypes.c_uint32, ctypes.c_uint32, U, P, P]),
        "pd_reduce_windows": (I, [P, ctypes.c_uint32, ctypes.c_uint32, P, P]),
        "pd_scan_depth_histogram": (I, [P, ctypes.c_uint32, U, P]),
        "pd_depth_histogram": (I, [P, P, SZ, ctypes.c_uint32, P]),
        "pd_depth_levels": (I, [P, ctypes.c_int32, ctypes.c_uint32, SZ, P, ctypes.c_uint32, P, SZ, ctypes.POINTER(SZ)]),
        "pd_depth_quantiles": (I, [P, P, SZ, P, SZ, P, ctypes.c_uint32, P, P]),
        "pd_window_quantiles": (I, [P, ctypes.c_uint32, P, ctypes.c_uint32, P]),
        "pd_depth_thresholds": (I, [P, P, SZ, P, SZ, P, ctypes.c_uint32, P, P]),
        "pd_window_thresholds": (I, [P, ctypes.c_uint32, P, ctypes.c_uint32, P]),
        "pd_depth_gc_bias": (I, [P, P, SZ, ctypes.c_uint32, P, P, P, P, P]),
        "pd_read_depth": (I, [P, ctypes.c_int32, ctypes.c_uint32, SZ, P]),
        "pd_format_sites": (I, [P, ctypes.c_int32, ctypes.c_uint32, SZ, ctypes.c_char_p, SZ, P, SZ, ctypes.POINTER(SZ)]),
        "pd_deflate_parse": (I, [P, P, SZ, P, ctypes.c_uint32, P, SZ, P]),
        "pd_host_register": (I, [P, P, SZ]),
        "pd_host_unregister": (I, [P, P]),
        "pd_text_open": (I, [P, SZ, ctypes.POINTER(P)]),
        "pd_text_close": (I, [P]),
        "pd_text_append_sites": (I, [P, ctypes.c_int32, ctypes.c_uint32, SZ, ctypes.c_char_p, SZ, ctypes.POINTER(ctypes.c_uint64)]),
        "pd_text_parse": (I, [P, ctypes.c_uint64, SZ, P, ctypes.c_uint32, P, SZ, P, P, ctypes.c_uint64]),
        "pd_text_read": (I, [P, ctypes.c_uint64, SZ, P]),
        "pd_text_release": (I, [P, ctypes.c_uint64]),
        "pd_text_append_window_rows": (I, [P, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, SZ, ctypes.c_char_p, SZ, ctypes.POINTER(ctypes.c_uint64)]),
        "pd_text_append_bytes": (I, [P, P, SZ]),
        "pd_device_buffer": (I, [P, ctypes.POINTER(P), ctypes.POINTER(U64), P]),
        "pd_device_count": (I, [ctypes.POINTER(I)]),
        "pd_accumulate_from": (I, [P, P]),
        "pd_device_layout": (I, [P, ctypes.POINTER(U64), ctypes.POINTER(U64)]),
        "pd_export_i8": (I, [P, I, P, P, ctypes.c_uint32, P]),
        "pd_import_i8": (I, [P, P, I, P, U64]),
        "pd_export_i4": (I, [P, P, P, ctypes.c_uint32, P]),
        "pd_slice_sweep_i4": (I, [P, P, ctypes.c_uint32, U64, U64, U64, P, P, U64, P, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_uint, P]),
        "pd_gather_windows": (I, [P, P, ctypes.c_uint32, P, P]),
        "pd_comm_unique_id": (I, [P]),
        "pd_comm_init": (I, [P, P, I, I, ctypes.POINTER(P)]),
        "pd_comm_init_all": (I, [ctypes.POINTER(P), I, ctypes.POINTER(P)]),
        "pd_comm_init_local": (I, [ctypes.POINTER(P), I, ctypes.POINTER(P)]),
        "pd_comm_preinit": (I, [ctypes.POINTER(I), I]),
        "pd_comm_destroy": (I, [P]),
        "pd_comm_prepare": (I, [P, I]),
        "pd_comm_strerror": (ctypes.c_char_p, [P]),
        "pd_sliced_window_sum": (I, [P, ctypes.c_uint32, ctypes.c_uint32, U, I, P, P]),
        "pd_sliced_interval_sum": (I, [P, P, SZ, ctypes.c_uint32, U, I, P, P]),
        "pd_sliced_sum_start": (I, [P, I]),
        "pd_sliced_sum_finish": (I, [P, I, ctypes.c_uint32, ctypes.c_uint32, U, I, P, P]),
        "pd_push_bgzf_units": (I, [P, P, SZ, P, ctypes.c_uint32, P, ctypes.c_uint32, U64, ctypes.c_uint32, ctypes.c_int32, P,
                               ctypes.POINTER(U64)]),
        "pd_decode_begin": (I, [P, ctypes.POINTER(pd_decode_cfg)]),
        "pd_decode_acquire": (I, [P, SZ, ctypes.POINTER(P)]),
        "pd_decode_submit": (I, [P, ctypes.POINTER(pd_decode_batch), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(pd_decode_result)]),
        "pd_decode_queue": (I, [P, ctypes.POINTER(pd_decode_batch), ctypes.POINTER(U64)]),
        "pd_decode_collect": (I, [P, U64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(pd_decode_result)]),
        "pd_decode_end": (I, [P]),
        "pd_decode_abort": (I, [P]),
        "pd_decode_record_stats": (I, [P, ctypes.POINTER(U64), SZ, ctypes.POINTER(U64)]),
        "pd_decode_row_bins": (I, [P, ctypes.c_uint32, ctypes.POINTER(U64), ctypes.POINTER(ctypes.c_uint32)]),
        "pd_decode_row_counts": (I, [P, ctypes.POINTER(U64), SZ]),
        "pd_decode_aln_stats": (I, [P, ctypes.POINTER(U64), SZ]),
        "pd_x_bgzf_inflate": (I, [I, P, SZ, P, SZ, ctypes.POINTER(SZ), I, I, ctypes.POINTER(ctypes.c_double),
                              ctypes.POINTER(ctypes.c_uint32)]),
        "pd_stream": (P, [P]),
        "pd_synchronize": (I, [P]),
        "pd_profile": (I, [P, I]),
        "pd_profile_get": (I, [P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(U64)]),
        "pd_guard_check": (I, [ctypes.c_char_p, SZ]),
        "pd_guard_selftest": (I, []),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    _LIB = L
    return L


EXPORTS = ["pd_abi_version", "pd_create", "pd_destroy", "pd_strerror", "pd_reset", "pd_push_intervals",
           "pd_push_intervals_device", "pd_runs_create", "pd_runs_destroy", "pd_push_runs", "pd_stage_acquire", "pd_stage_submit", "pd_set_param", "pd_keep_deferred", "pd_scan",
           "pd_reduce_intervals", "pd_window_layout", "pd_scan_reduce_windows", "pd_reduce_windows", "pd_scan_depth_histogram", "pd_depth_histogram", "pd_depth_levels", "pd_depth_quantiles", "pd_window_quantiles", "pd_depth_thresholds", "pd_window_thresholds", "pd_depth_gc_bias",
           "pd_read_depth", "pd_format_sites", "pd_deflate_parse", "pd_host_register", "pd_host_unregister", "pd_text_open", "pd_text_close", "pd_text_append_sites", "pd_text_parse", "pd_text_read", "pd_text_release", "pd_text_append_window_rows", "pd_text_append_bytes", "pd_device_buffer", "pd_device_count", "pd_accumulate_from", "pd_device_layout", "pd_export_i8", "pd_import_i8", "pd_export_i4",
           "pd_slice_sweep_i4", "pd_gather_windows", "pd_push_bgzf_units", "pd_decode_begin", "pd_decode_acquire", "pd_decode_submit", "pd_decode_queue", "pd_decode_collect", "pd_decode_end", "pd_decode_abort", "pd_decode_record_stats", "pd_decode_row_bins", "pd_decode_row_counts", "pd_decode_aln_stats", "pd_comm_unique_id", "pd_comm_init", "pd_comm_init_all", "pd_comm_init_local", "pd_comm_preinit", "pd_comm_prepare", "pd_comm_destroy",
           "pd_comm_strerror", "pd_sliced_window_sum", "pd_sliced_interval_sum", "pd_sliced_sum_start", "pd_sliced_sum_finish", "pd_x_bgzf_inflate", "pd_stream", "pd_synchronize", "pd_profile",
           "pd_profile_get", "pd_guard_check", "pd_guard_selftest", "pd_runs_pileup_tiles"]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def as_iv(a):
    """(n,3) int32 array or IV_DTYPE array -> contiguous (n,3) int32."""
    a = np.asarray(a)
    if a.dtype == IV_DTYPE:
        a = a.view(np.int32).reshape(-1, 3)
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 3)


def bgzf_inflate(data, variant=0, reps=1, device=0, want_output=True):
    """pd_x_bgzf_inflate: returns (bytes or None, kernel_ms, n_blocks)."""
    L = load()
    buf = np.frombuffer(data, dtype=np.uint8)
    n = ctypes.c_size_t()
    ms = ctypes.c_double()
    nb = ctypes.c_uint32()
    # exact output size from the ISIZE trailers of the blocks
    cap, o = 64, 0
    while o + 18 <= buf.size:
        bs = int(buf[o + 16]) + (int(buf[o + 17]) << 8) + 1
        cap += int.from_bytes(bytes(buf[o + bs - 4:o + bs]), "little")
        o += bs
    out = np.empty(cap if want_output else 1, dtype=np.uint8)
    rc = L.pd_x_bgzf_inflate(int(device), _ptr(buf), buf.size, _ptr(out) if want_output else None, out.size if want_output else 0,
                             ctypes.byref(n), int(variant), int(reps), ctypes.byref(ms), ctypes.byref(nb))
    if rc != 0:
        raise PdError(rc, "pd_x_bgzf_inflate failed")
    return (out[:n.value].tobytes() if want_output else None), float(ms.value), int(nb.value), int(n.value)


PD_UNIQUE_ID_BYTES = 128


def comm_unique_id():
    """pd_comm_unique_id: the 128 bytes one rank makes and every rank passes to Comm()."""
    b = ctypes.create_string_buffer(PD_UNIQUE_ID_BYTES)
    rc = load().pd_comm_unique_id(b)
    if rc != 0:
        raise PdError(rc, "pd_comm_unique_id failed (librccl?)")
    return b.raw


class Comm:
    """One pd_comm: this rank's end of the RCCL sliced sum (the collectives are issued inside the library)."""

    def __init__(self, engine, unique_id, rank, world):
        self.L, self.e, self.rank, self.world = engine.L, engine, int(rank), int(world)
        h = ctypes.c_void_p()
        rc = self.L.pd_comm_init(engine.h, ctypes.c_char_p(bytes(unique_id)), self.rank, self.world, ctypes.byref(h))
        if rc != 0:
            raise PdError(rc, (self.L.pd_strerror(engine.h) or b"").decode())
        self.h = h

    @classmethod
    def local(cls, engines):
        """pd_comm_init_local: one communicator per engine of THIS process (threads as ranks), no RCCL — the executable's `#.list`
        transport.  Returns the list of Comm objects, rank k on engines[k]."""
        n = len(engines)
        L = engines[0].L
        ctxs = (ctypes.c_void_p * n)(*[e.h for e in engines])
        out = (ctypes.c_void_p * n)()
        rc = L.pd_comm_init_local(ctxs, n, out)
        if rc != 0:
            raise PdError(rc, (L.pd_strerror(engines[0].h) or b"").decode())
        comms = []
        for k, e in enumerate(engines):
            c = cls.__new__(cls)
            c.L, c.e, c.rank, c.world, c.h = L, e, k, n, ctypes.c_void_p(out[k])
            comms.append(c)
        return comms

    def _ck(self, rc):
        if rc != 0:
            raise PdError(rc, (self.L.pd_comm_strerror(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.e, "h", None):          # (a context that is already gone took its stream along: nothing left to release safely)
                self.L.pd_comm_destroy(self.h)
            self.h = None

    __del__ = close

    def start(self, slot=0):
        self._ck(self.L.pd_sliced_sum_start(self.h, int(slot)))

    def finish(self, slot=0, w=10000000, min_dep=1, wrap_bits=18, root=0):
        """(win_off, cover, depth_sum) on the root, else None."""
        if self.rank != root:
            self._ck(self.L.pd_sliced_sum_finish(self.h, int(slot), int(w), int(min_dep), int(wrap_bits), int(root), None, None))
            return None
        off = self.e.window_layout(w)
        n = int(off[-1])
        cover = np.zeros(max(n, 1), dtype=np.uint32)
        tot = np.zeros(max(n, 1), dtype=np.uint64)
        self._ck(self.L.pd_sliced_sum_finish(self.h, int(slot), int(w), int(min_dep), int(wrap_bits), int(root), _ptr(cover), _ptr(tot)))
        return off, cover[:n], tot[:n]

    def run(self, w=10000000, min_dep=1, wrap_bits=18, root=0):
        self.start(0)
        return self.finish(0, w, min_dep, wrap_bits, root)

    def window_sum(self, w, min_dep=1, wrap_bits=18, root=0):
        """pd_sliced_window_sum (any window width): (win_off, cover, depth_sum) on the root, else None."""
        if self.rank != root:
            self._ck(self.L.pd_sliced_window_sum(self.h, int(w), int(min_dep), int(wrap_bits), int(root), None, None))
            return None
        off = self.e.window_layout(w)
        n = int(off[-1])
        cover = np.zeros(max(n, 1), dtype=np.uint32)
        tot = np.zeros(max(n, 1), dtype=np.uint64)
        self._ck(self.L.pd_sliced_window_sum(self.h, int(w), int(min_dep), int(wrap_bits), int(root), _ptr(cover), _ptr(tot)))
        return off, cover[:n], tot[:n]

    def interval_sum(self, regs, min_dep=1, wrap_bits=18, root=0):
        """pd_sliced_interval_sum: (cover, depth_sum) per region on the root, else None."""
        regs = np.ascontiguousarray(regs, dtype=np.int32).reshape(-1, 3)
        n = regs.shape[0]
        if self.rank != root:
            self._ck(self.L.pd_sliced_interval_sum(self.h, _ptr(regs), n, int(min_dep), int(wrap_bits), int(root), None, None))
            return None
        cover = np.zeros(max(n, 1), dtype=np.int32)
        tot = np.zeros(max(n, 1), dtype=np.uint64)
        self._ck(self.L.pd_sliced_interval_sum(self.h, _ptr(regs), n, int(min_dep), int(wrap_bits), int(root), _ptr(cover), _ptr(tot)))
        return cover[:n], tot[:n]


class Engine:
    """One pd_ctx.  Method names follow the C entry points without the pd_ prefix."""

    def __init__(self, contig_len, device=0):
        self.L = load()
        self.len = np.ascontiguousarray(contig_len, dtype=np.uint32)
        self.n_contigs = int(self.len.size)
        h = ctypes.c_void_p()
        rc = self.L.pd_create(int(device), self.n_contigs, _ptr(self.len), ctypes.byref(h))
        if rc != 0:
            raise PdError(rc, (self.L.pd_strerror(None) or b"").decode())
        self.h = h

    def _ck(self, rc):
        if rc != 0:
            raise PdError(rc, (self.L.pd_strerror(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.pd_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        self._ck(self.L.pd_reset(self.h))

    def keep_deferred(self, enable=True):
        self._ck(self.L.pd_keep_deferred(self.h, 1 if enable else 0))

    def set_param(self, name, value):
        self._ck(self.L.pd_set_param(self.h, name.encode(), int(value)))

    def push_intervals(self, iv, flags=PD_PUSH_DEFAULT):
        iv = as_iv(iv)
        self._ck(self.L.pd_push_intervals(self.h, _ptr(iv), iv.shape[0], int(flags)))

    def push_intervals_device(self, dev_ptr, n, flags=PD_PUSH_DEFAULT):
        self._ck(self.L.pd_push_intervals_device(self.h, ctypes.c_void_p(int(dev_ptr)), int(n), int(flags)))

    def runs_create(self, sorted_ptr, n_sorted, other_ptr=0, n_other=0):
        """A device-resident sample — runs sorted by (tid, beg) + further runs in any order — as ONE compact sample
        (pd_runs_create); PdError(-1) if the first batch is not sorted."""
        h = ctypes.c_void_p()
        self._ck(self.L.pd_runs_create(self.h, ctypes.c_void_p(int(sorted_ptr)), int(n_sorted), ctypes.c_void_p(int(other_ptr)) if n_other else None,
                                       int(n_other), ctypes.byref(h)))
        return h

    def runs_destroy(self, runs):
        self._ck(self.L.pd_runs_destroy(runs))

    def push_runs(self, runs, flags=PD_PUSH_MORE):
        self._ck(self.L.pd_push_runs(self.h, runs, int(flags)))

    def runs_pileup_tiles(self, runs=None):
        """The pile-up tiles a compact sample listed at its making, sorted (runs=None: the decode session's sample).
        (Its signature is set here, not in load(): a tuning library from before the entry point still loads.)"""
        f = self.L.pd_runs_pileup_tiles
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        n = ctypes.c_uint32(0)
        self._ck(f(self.h, runs, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self._ck(f(self.h, runs, _ptr(out), n.value, ctypes.byref(n)))
        return np.sort(out)

    def deflate_parse(self, text, chunks):
        """zlib's level-6 LZ77 parse of the chunks [(start, end, origin), ...] of `text` (bytes / uint8 array) on the device:
        a list of uint32 symbol arrays (literal = byte, match = len << 16 | dist), one per chunk."""
        t = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, dtype=np.uint8)
        ch = np.ascontiguousarray(np.asarray(chunks, dtype=np.uint64).reshape(-1, 3))
        cap = int(sum(int(e - s) for s, e, _ in ch.tolist())) + 16
        syms = np.zeros(cap, dtype=np.uint32)
        off = np.zeros(ch.shape[0] + 1, dtype=np.uint64)
        self._ck(self.L.pd_deflate_parse(self.h, _ptr(t), t.size, _ptr(ch), ch.shape[0], _ptr(syms), cap, _ptr(off)))
        return [syms[int(off[k]):int(off[k + 1])] for k in range(ch.shape[0])]

    def scan(self, wrap_bits=0):
        self._ck(self.L.pd_scan(self.h, int(wrap_bits)))

    def reduce_intervals(self, regs, min_dep=1):
        regs = np.ascontiguousarray(regs, dtype=np.int32).reshape(-1, 3)
        n = regs.shape[0]
        cover = np.zeros(n, dtype=np.int32)
        tot = np.zeros(n, dtype=np.uint64)
        self._ck(self.L.pd_reduce_intervals(self.h, _ptr(regs), n, int(min_dep), _ptr(cover), _ptr(tot)))
        return cover, tot

    def window_layout(self, w):
        off = np.zeros(self.n_contigs + 1, dtype=np.uint64)
        self._ck(self.L.pd_window_layout(self.h, int(w), _ptr(off)))
        return off

    def scan_reduce_windows(self, w, min_dep=1, wrap_bits=0):
        off = self.window_layout(w)
        n = int(off[-1])
        cover = np.zeros(max(n, 1), dtype=np.uint32)
        tot = np.zeros(max(n, 1), dtype=np.uint64)
        self._ck(self.L.pd_scan_reduce_windows(self.h, int(w), int(min_dep), int(wrap_bits), _ptr(cover), _ptr(tot)))
        return off, cover[:n], tot[:n]

    def reduce_windows(self, w, min_dep=1, out=None):
        """out = (cover uint32 array, sum uint64 array) of at least pd_window_layout(w)[-1] entries to receive the results (a caller
        with millions of windows keeps its arrays: fresh pages cost more than the copy)."""
        off = self.window_layout(w)
        n = int(off[-1])
        if out is not None:
            cover, tot = out
            assert cover.dtype == np.uint32 and tot.dtype == np.uint64 and cover.size >= n and tot.size >= n
        else:
            cover = np.zeros(max(n, 1), dtype=np.uint32)
            tot = np.zeros(max(n, 1), dtype=np.uint64)
        self._ck(self.L.pd_reduce_windows(self.h, int(w), int(min_dep), _ptr(cover), _ptr(tot)))
        return off, cover[:n], tot[:n]

    def scan_depth_histogram(self, n_bins, wrap_bits=0):
        """pd_scan_depth_histogram: (n_contigs, n_bins) uint64, row t = contig t's cells by depth (last bin: depth >= n_bins - 1),
        fused over the difference arrays (the context stays accumulating)."""
        hist = np.zeros((max(self.n_contigs, 1), int(n_bins)), dtype=np.uint64)
        self._ck(self.L.pd_scan_depth_histogram(self.h, int(n_bins), int(wrap_bits), _ptr(hist)))
        return hist[:self.n_contigs]

    def depth_histogram(self, n_bins, regs=None):
        """pd_depth_histogram after scan: whole contigs (regs None / empty) or the cells [first-1, second) of regions (n, 3) int32
        (tid, first, second), sorted by (tid, first) and disjoint; (n_contigs, n_bins) uint64."""
        hist = np.zeros((max(self.n_contigs, 1), int(n_bins)), dtype=np.uint64)
        if regs is None or len(regs) == 0:
            self._ck(self.L.pd_depth_histogram(self.h, None, 0, int(n_bins), _ptr(hist)))
        else:
            r = np.ascontiguousarray(regs, dtype=np.int32).reshape(-1, 3)
            self._ck(self.L.pd_depth_histogram(self.h, _ptr(r), r.shape[0], int(n_bins), _ptr(hist)))
        return hist[:self.n_contigs]

    def depth_levels(self, tid, beg=0, n=None, edges=None, cap=None):
        """pd_depth_levels after scan: the cells [beg, beg + n) of contig tid as maximal runs, (n_levels, 2) uint32 rows
        (start, value); value = the depth (edges None / empty) or the index of the depth's class among the ascending edges
        (0xFFFFFFFF below edges[0]).  cap (default n) bounds the rows the library may write."""
        if n is None:
            n = int(self.len[tid]) - int(beg)
        cap = int(n) if cap is None else int(cap)
        out = np.empty((max(cap, 1), 2), dtype=np.uint32)
        got = ctypes.c_size_t(0)
        if edges is None or len(edges) == 0:
            e, ne = None, 0
        else:
            e = np.ascontiguousarray(edges, dtype=np.uint32)
            ne = int(e.shape[0])
        self._ck(self.L.pd_depth_levels(self.h, int(tid), int(beg), int(n), None if e is None else _ptr(e), ne, _ptr(out), cap, ctypes.byref(got)))
        return out[:got.value]

    def depth_quantiles(self, segs, row_off, pct):
        """pd_depth_quantiles after scan: row i = the segments segs[row_off[i]:row_off[i + 1]] ((n, 3) int32: tid, first, second —
        cells [first-1, second) clipped to the contig, a multiset); returns (cells uint64 (n_rows,), q uint32 (n_rows, len(pct))),
        q[i, j] = the nearest-rank pct[j] percentile of row i's cells, 0xFFFFFFFF for a row without cells."""
        sg = np.ascontiguousarray(segs, dtype=np.int32).reshape(-1, 3)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        pc = np.ascontiguousarray(pct, dtype=np.uint32)
        n_rows, npc = int(ro.size) - 1, int(pc.size)
        cells = np.zeros(max(n_rows, 1), dtype=np.uint64)
        q = np.zeros((max(n_rows, 1), max(npc, 1)), dtype=np.uint32)
        pcb = pc if npc else np.zeros(1, dtype=np.uint32)
        self._ck(self.L.pd_depth_quantiles(self.h, _ptr(sg) if sg.shape[0] else None, sg.shape[0], _ptr(ro), n_rows, _ptr(pcb), npc, _ptr(cells), _ptr(q)))
        return cells[:n_rows], q[:n_rows]

    def window_quantiles(self, w, pct):
        """pd_window_quantiles after scan: (win_off, q uint32 (n_windows, len(pct))) for the windows of window_layout(w)."""
        off = self.window_layout(w)
        n = int(off[-1])
        pc = np.ascontiguousarray(pct, dtype=np.uint32)
        npc = int(pc.size)
        q = np.zeros((max(n, 1), max(npc, 1)), dtype=np.uint32)
        pcb = pc if npc else np.zeros(1, dtype=np.uint32)
        self._ck(self.L.pd_window_quantiles(self.h, int(w), _ptr(pcb), npc, _ptr(q)))
        return off, q[:n]

    def depth_thresholds(self, segs, row_off, thr):
        """pd_depth_thresholds after scan: rows as in depth_quantiles; returns (cells uint64 (n_rows,), counts uint64
        (n_rows, len(thr))), counts[i, j] = the number of cells of row i that are >= thr[j] (zeros for a row without cells)."""
        sg = np.ascontiguousarray(segs, dtype=np.int32).reshape(-1, 3)
        ro = np.ascontiguousarray(row_off, dtype=np.uint64)
        th = np.ascontiguousarray(thr, dtype=np.uint32)
        n_rows, nt = int(ro.size) - 1, int(th.size)
        cells = np.zeros(max(n_rows, 1), dtype=np.uint64)
        counts = np.zeros((max(n_rows, 1), max(nt, 1)), dtype=np.uint64)
        thb = th if nt else np.zeros(1, dtype=np.uint32)
        self._ck(self.L.pd_depth_thresholds(self.h, _ptr(sg) if sg.shape[0] else None, sg.shape[0], _ptr(ro), n_rows, _ptr(thb), nt, _ptr(cells), _ptr(counts)))
        return cells[:n_rows], counts[:n_rows]

    def window_thresholds(self, w, thr):
        """pd_window_thresholds after scan: (win_off, counts uint32 (n_windows, len(thr))) for the windows of window_layout(w)."""
        off = self.window_layout(w)
        n = int(off[-1])
        th = np.ascontiguousarray(thr, dtype=np.uint32)
        nt = int(th.size)
        counts = np.zeros((max(n, 1), max(nt, 1)), dtype=np.uint32)
        thb = th if nt else np.zeros(1, dtype=np.uint32)
        self._ck(self.L.pd_window_thresholds(self.h, int(w), _ptr(thb), nt, _ptr(counts)))
        return off, counts[:n]

    def depth_gc_bias(self, w, bases, regs=None):
        """pd_depth_gc_bias after scan: windows of w cells tiled from the first cell of every contig (regs None / empty) or of
        every region ((n, 3) int32: tid, first, second; sorted by (tid, first), disjoint).  bases: one bytes-like object (bytes,
        uint8 array) or None per contig.  Returns (windows uint64 (101,), sum uint64 (101,), skipped int)."""
        keep = [None if b is None else np.ascontiguousarray(np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray)) else b, dtype=np.uint8)
                for b in bases]
        assert len(keep) == self.n_contigs
        ptrs = (ctypes.c_void_p * max(self.n_contigs, 1))(*[None if b is None else b.ctypes.data for b in keep])
        nb = np.array([0 if b is None else b.size for b in keep] + [0], dtype=np.uint32)
        windows = np.zeros(101, dtype=np.uint64)
        tot = np.zeros(101, dtype=np.uint64)
        skipped = ctypes.c_uint64(0)
        if regs is None or len(regs) == 0:
            r, n = None, 0
        else:
            r = np.ascontiguousarray(regs, dtype=np.int32).reshape(-1, 3)
            n = r.shape[0]
        self._ck(self.L.pd_depth_gc_bias(self.h, None if r is None else _ptr(r), n, int(w), ctypes.cast(ptrs, ctypes.c_void_p), _ptr(nb), _ptr(windows), _ptr(tot),
                                         ctypes.cast(ctypes.byref(skipped), ctypes.c_void_p)))
        return windows, tot, int(skipped.value)

    def read_depth(self, tid, beg=0, n=None):
        if n is None:
            n = int(self.len[tid]) - int(beg)
        out = np.zeros(max(int(n), 1), dtype=np.uint32)
        self._ck(self.L.pd_read_depth(self.h, int(tid), int(beg), int(n), _ptr(out)))
        return out[:int(n)]

    def device_buffer(self):
        p = ctypes.c_void_p()
        nw = ctypes.c_uint64()
        off = np.zeros(self.n_contigs, dtype=np.uint64)
        self._ck(self.L.pd_device_buffer(self.h, ctypes.byref(p), ctypes.byref(nw), _ptr(off)))
        return int(p.value), int(nw.value), off

    def accumulate_from(self, other):
        self._ck(self.L.pd_accumulate_from(self.h, other.h))

    def format_sites(self, tid, beg, n, name):
        """pd_format_sites: bytes of the per-site rows of cells [beg, beg + n) of contig tid."""
        nm = name.encode() if isinstance(name, str) else bytes(name)
        buf = np.empty(max(1, int(n) * (len(nm) + 23)), dtype=np.uint8)
        got = ctypes.c_size_t()
        self._ck(self.L.pd_format_sites(self.h, int(tid), int(beg), int(n), nm, len(nm), _ptr(buf), buf.size, ctypes.byref(got)))
        return buf[:got.value].tobytes()

    def text_open(self, capacity):
        """A device-resident text stream (pd_text_*): see TextStream."""
        return TextStream(self, capacity)

    def device_layout(self):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._ck(self.L.pd_device_layout(self.h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def export_i8(self, threshold, i8_ptr, exc_ptr, exc_cap, count_ptr):
        self._ck(self.L.pd_export_i8(self.h, int(threshold), ctypes.c_void_p(int(i8_ptr)), ctypes.c_void_p(int(exc_ptr)),
                                     int(exc_cap), ctypes.c_void_p(int(count_ptr))))

    def import_i8(self, i8_ptr, bias, exc_ptr, n_exc):
        self._ck(self.L.pd_import_i8(self.h, ctypes.c_void_p(int(i8_ptr)), int(bias),
                                     ctypes.c_void_p(int(exc_ptr) if n_exc else 0), int(n_exc)))

    def export_i4(self, i4_ptr, exc_ptr, exc_cap, count_ptr):
        self._ck(self.L.pd_export_i4(self.h, ctypes.c_void_p(int(i4_ptr)), ctypes.c_void_p(int(exc_ptr)), int(exc_cap),
                                     ctypes.c_void_p(int(count_ptr))))

    def slice_sweep_i4(self, parts_ptr, n_parts, part_stride, tile_first, tile_count, tile_sums_ptr, exc_ptr, exc_stride,
                       exc_counts_ptr, w, min_dep, wrap_bits, partials_ptr):
        self._ck(self.L.pd_slice_sweep_i4(self.h, ctypes.c_void_p(int(parts_ptr)), int(n_parts), int(part_stride),
                                          int(tile_first), int(tile_count), ctypes.c_void_p(int(tile_sums_ptr)),
                                          ctypes.c_void_p(int(exc_ptr) or None), int(exc_stride),
                                          ctypes.c_void_p(int(exc_counts_ptr) or None), int(w), int(min_dep),
                                          int(wrap_bits), ctypes.c_void_p(int(partials_ptr))))

    def gather_windows(self, partials_ptr, w):
        off = self.window_layout(w)
        n = int(off[-1])
        cover = np.zeros(max(n, 1), dtype=np.uint32)
        tot = np.zeros(max(n, 1), dtype=np.uint64)
        self._ck(self.L.pd_gather_windows(self.h, ctypes.c_void_p(int(partials_ptr)), int(w), _ptr(cover), _ptr(tot)))
        return off, cover[:n], tot[:n]

    def push_bgzf_units(self, blob, blocks, units, inflated_bytes, flag_mask=1796, min_mapq=-1, count_deletions=False, fragments=False, frag_max=0):
        """blocks: (n,4) uint64-compatible rows {in_off, out_off, in_len, out_len}; units: rows
        {start, stop, avail, first_block, n_blocks}.  Returns (unit_status int32 array, n_records).
        count_deletions: deletions count as covered (PD_DECODE_DELETIONS).  The C entry takes it from the parameter "decode_deletions",
        which every call here sets to this argument's value: the argument alone decides, whatever set_param left there.
        fragments, frag_max: whole fragments of properly paired reads (PD_DECODE_FRAGMENTS) and the bound on |tlen| (0: none), by the
        parameters "decode_fragments" and "decode_frag_max" in the same way."""
        blob = np.frombuffer(blob, dtype=np.uint8)
        bd = np.zeros(len(blocks), dtype=np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_len", "<u4")]))
        for k, name in enumerate(("in_off", "out_off", "in_len", "out_len")):
            bd[name] = [b[k] for b in blocks]
        ud = np.zeros(len(units), dtype=np.dtype([("start", "<u8"), ("stop", "<u8"), ("avail", "<u8"), ("first_block", "<u4"),
                                                   ("n_blocks", "<u4")]))
        for k, name in enumerate(("start", "stop", "avail", "first_block", "n_blocks")):
            ud[name] = [u[k] for u in units]
        st = np.zeros(max(1, len(units)), dtype=np.int32)
        nrec = ctypes.c_uint64()
        self.set_param("decode_deletions", 1 if count_deletions else 0)
        self.set_param("decode_fragments", 1 if fragments else 0)
        self.set_param("decode_frag_max", int(frag_max))
        self._ck(self.L.pd_push_bgzf_units(self.h, _ptr(blob), blob.size, _ptr(bd), len(blocks), _ptr(ud), len(units),
                                           int(inflated_bytes), int(flag_mask), int(min_mapq), _ptr(st), ctypes.byref(nrec)))
        return st[:len(units)], int(nrec.value)

    def decode_session(self):
        """The pd_decode_* calls of this context: see DecodeSession."""
        return DecodeSession(self)

    def stream(self):
        return int(self.L.pd_stream(self.h) or 0)

    def synchronize(self):
        self._ck(self.L.pd_synchronize(self.h))

    def profile(self, enable=True):
        self._ck(self.L.pd_profile(self.h, 1 if enable else 0))

    def profile_get(self, name):
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        self._ck(self.L.pd_profile_get(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)


class DecodeSession:
    """pd_decode_begin / acquire / submit / queue / collect / end / abort on one Engine, one method per call and nothing between them.
    A batch is the tuple (bytes, blocks, units, inflated_bytes, order): blocks rows (in_off, out_off, in_len, out_len), units rows
    (start, stop, avail, first_block, n_blocks[, flags]).  `acquire` hands out a pinned buffer; `submit` / `queue` copy the batch's
    bytes into the buffer given (default: the one acquired longest ago and not yet used).  `submit` and `collect` return
    (unit_status int32 array, result dict of pd_decode_result's fields).  A call that fails raises PdError, which leaves the session
    as the library left it."""

    def __init__(self, eng):
        self.e, self.L = eng, eng.L
        self.n_isize = 0                     # begin's record_stats (the insert bins of pd_decode_record_stats)
        self.n_row_bins = 0                  # begin's row_counts (the bins of pd_decode_row_counts)
        self._keep = []                      # arrays the C side reads during a call (and, for begin, until it returns)
        self.held = []                       # buffers acquired and not yet handed to submit / queue

    def begin(self, flag_mask=1796, min_mapq=-1, contig_on=None, span_off=None, spans=None, sorted=1, bytes_hint=0, batch_bytes=0,
              batches_in_flight=0, flags=0, n_batches=0, count_deletions=False, fragments=False, frag_max=0, record_stats=0, row_counts=None, aln_stats=0):
        """record_stats=N (1 .. 65536) adds PD_DECODE_RECORD_STATS: the session also counts its records, with N insert bins (the parameter
        "decode_isize_bins"); record_stats() returns the numbers after end().
        row_counts=("w", W) or ("edges", edge_off, edges) adds PD_DECODE_ROW_COUNTS: the session also counts its records per bin of that table
        (pd_decode_row_bins, set here; edge_off None: no edges, one bin per contig); row_counts() returns the bins after end().
        aln_stats=W (1 .. 65536) adds PD_DECODE_ALN_STATS: the session also sums its records' CIGAR operations and read lengths, in length bins
        of W bases (the parameter "decode_len_bin_width"); aln_stats() returns the numbers after end().
        count_deletions adds PD_DECODE_DELETIONS to `flags`: deletions count as covered, one run per group of M/=/X/D operations.
        fragments adds PD_DECODE_FRAGMENTS: a properly paired read with tlen > 0 is the one run [pos, pos + tlen), its mate none; frag_max
        bounds |tlen| (0: no bound).  The bound travels as the parameter "decode_frag_max", set here from the argument at every call."""
        if count_deletions:
            flags = int(flags) | PD_DECODE_DELETIONS
        if fragments:
            flags = int(flags) | PD_DECODE_FRAGMENTS
        self.e.set_param("decode_frag_max", int(frag_max))
        self.n_isize = int(record_stats)
        if record_stats:
            flags = int(flags) | PD_DECODE_RECORD_STATS
            self.e.set_param("decode_isize_bins", int(record_stats))
        if aln_stats:
            flags = int(flags) | PD_DECODE_ALN_STATS
            self.e.set_param("decode_len_bin_width", int(aln_stats))
        if row_counts is not None:
            flags = int(flags) | PD_DECODE_ROW_COUNTS
            self.n_row_bins = self.row_bins(*row_counts)
        cfg = pd_decode_cfg()
        cfg.flag_mask, cfg.min_mapq, cfg.sorted = int(flag_mask), int(min_mapq), int(sorted)
        cfg.bytes_hint, cfg.batch_bytes, cfg.batches_in_flight, cfg.flags, cfg.n_batches = int(bytes_hint), int(batch_bytes), int(batches_in_flight), int(flags), int(n_batches)
        keep = [cfg]
        if contig_on is not None:
            on = np.ascontiguousarray(contig_on, dtype=np.uint8)
            assert on.size == self.e.n_contigs
            keep.append(on); cfg.contig_on = on.ctypes.data
        if (spans is None) != (span_off is None):
            raise ValueError("span_off and spans go together (spans of contig t are spans[span_off[t]:span_off[t + 1]])")
        if spans is not None:
            so = np.ascontiguousarray(span_off, dtype=np.uint32)
            sp = np.ascontiguousarray(np.asarray(spans, dtype=np.int32).reshape(-1, 2))
            assert so.size == self.e.n_contigs + 1 and int(so[-1]) == sp.shape[0]
            pad = np.zeros((max(sp.shape[0], 1), 2), dtype=np.int32)         # (never a NULL pointer for an empty list: NULL means "every read")
            pad[:sp.shape[0]] = sp
            keep += [so, pad]; cfg.span_off = so.ctypes.data; cfg.spans = pad.ctypes.data
        self._keep = keep
        self.e._ck(self.L.pd_decode_begin(self.e.h, ctypes.byref(cfg)))

    def acquire(self, nbytes):
        """-> the address of a pinned buffer of at least nbytes bytes (held until a batch is submitted or queued with it)"""
        p = ctypes.c_void_p()
        self.e._ck(self.L.pd_decode_acquire(self.e.h, int(nbytes), ctypes.byref(p)))
        self.held.append(int(p.value))
        return int(p.value)

    def _take(self, buf):
        if buf is None:
            buf = self.held[0]
        if buf in self.held:
            self.held.remove(buf)
        return buf

    def _batch(self, buf, batch):
        data, blocks, units, inflated, order = batch
        data = bytes(data)
        if data:
            ctypes.memmove(buf, data, len(data))
        nb, nu = len(blocks), len(units)
        bd = (pd_bgzf_block * max(nb, 1))()
        for k, b in enumerate(blocks):
            bd[k].in_off, bd[k].out_off, bd[k].in_len, bd[k].out_len = (int(x) for x in b[:4])
        ud = (pd_decode_unit * max(nu, 1))()
        for k, u in enumerate(units):
            ud[k].start, ud[k].stop, ud[k].avail, ud[k].first_block, ud[k].n_blocks = (int(x) for x in u[:5])
            ud[k].flags = int(u[5]) if len(u) > 5 else 0
        bt = pd_decode_batch()
        bt.host_buf, bt.n_bytes, bt.n_blocks, bt.n_units, bt.inflated_bytes, bt.order = buf, len(data), nb, nu, int(inflated), int(order)
        bt.blocks = ctypes.cast(bd, ctypes.POINTER(pd_bgzf_block)) if nb else None
        bt.units = ctypes.cast(ud, ctypes.POINTER(pd_decode_unit)) if nu else None
        return bt, (bd, ud)

    @staticmethod
    def _result(st, n_units, res):
        return np.array(st[:n_units], dtype=np.int32), {name: getattr(res, name) for name, _ in pd_decode_result._fields_ if name != "pad"}

    def submit(self, batch, buf=None):
        bt, keep = self._batch(self._take(buf), batch)
        st = (ctypes.c_int32 * max(bt.n_units, 1))()
        res = pd_decode_result()
        self.e._ck(self.L.pd_decode_submit(self.e.h, ctypes.byref(bt), st, ctypes.byref(res)))
        del keep
        return self._result(st, bt.n_units, res)

    def queue(self, batch, buf=None):
        """-> ticket (pd_decode_queue copies the batch's tables; the buffer stays the engine's until the batch is collected)"""
        bt, keep = self._batch(self._take(buf), batch)
        t = ctypes.c_uint64()
        self.e._ck(self.L.pd_decode_queue(self.e.h, ctypes.byref(bt), ctypes.byref(t)))
        del keep
        return int(t.value)

    def collect(self, ticket, n_units):
        st = (ctypes.c_int32 * max(int(n_units), 1))()
        res = pd_decode_result()
        self.e._ck(self.L.pd_decode_collect(self.e.h, int(ticket), st, ctypes.byref(res)))
        return self._result(st, int(n_units), res)

    def end(self):
        self.held = []
        self.e._ck(self.L.pd_decode_end(self.e.h))
        self._keep = []

    def abort(self):
        self.held = []
        self.e._ck(self.L.pd_decode_abort(self.e.h))
        self._keep = []

    def row_bins(self, form, *table):
        """pd_decode_row_bins: ("w", W) or ("edges", edge_off, edges) -> the number of bins of that table"""
        U64P, U32P = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
        if form == "w":
            w = int(table[0])
            self.e._ck(self.L.pd_decode_row_bins(self.e.h, w, None, None))
            return int(self.e.window_layout(w)[-1])
        assert form == "edges", form
        edge_off, edges = table
        if edge_off is None:
            self.e._ck(self.L.pd_decode_row_bins(self.e.h, 0, None, None))
            return self.e.n_contigs
        off = np.ascontiguousarray(edge_off, dtype=np.uint64)
        ed = np.ascontiguousarray(edges, dtype=np.uint32)
        assert off.size == self.e.n_contigs + 1
        self.e._ck(self.L.pd_decode_row_bins(self.e.h, 0, off.ctypes.data_as(U64P), ed.ctypes.data_as(U32P) if ed.size else None))
        return int(off[-1]) + self.e.n_contigs

    def row_counts(self):
        """pd_decode_row_counts -> uint64[n_bins, PD_ROWCOUNT_WORDS] (records, passed, mapq0, kept, forward, mapq_sum per bin) of the session
        that end() closed; PdError for a session begun without row_counts="""
        out = np.zeros((max(self.n_row_bins, 1), PD_ROWCOUNT_WORDS), dtype=np.uint64)
        self.e._ck(self.L.pd_decode_row_counts(self.e.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), self.n_row_bins))
        return out[:self.n_row_bins]

    def aln_stats(self):
        """pd_decode_aln_stats -> uint64[PD_ALNSTAT_WORDS] of the session that end() closed; PdError for a session begun without aln_stats=W"""
        sums = np.zeros(PD_ALNSTAT_WORDS, dtype=np.uint64)
        self.e._ck(self.L.pd_decode_aln_stats(self.e.h, sums.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), sums.size))
        return sums

    def record_stats(self):
        """pd_decode_record_stats -> (sums: uint64[PD_RECSTAT_FIXED + N + 1], per_contig: uint64[n_contigs, 3]) of the session that
        end() closed; PdError for a session begun without record_stats=N"""
        sums = np.zeros(PD_RECSTAT_FIXED + self.n_isize + 1, dtype=np.uint64)
        per = np.zeros((max(self.e.n_contigs, 1), 3), dtype=np.uint64)
        U64P = ctypes.POINTER(ctypes.c_uint64)
        self.e._ck(self.L.pd_decode_record_stats(self.e.h, sums.ctypes.data_as(U64P), sums.size, per.ctypes.data_as(U64P)))
        return sums, per[:self.e.n_contigs]


class TextStream:
    """pd_text_*: per-site rows formatted at the end of a stream that lives in HBM, parsed (zlib's LZ77 parse) and check-summed
    there; `append_sites` returns the bytes added (PdError(-6) when the ring has no room), `parse` a list of symbol arrays and the
    chunks' CRCs, `read` a stretch of the text."""

    def __init__(self, eng, capacity):
        self.e = eng
        self.h = ctypes.c_void_p()
        eng._ck(eng.L.pd_text_open(eng.h, int(capacity), ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.e.L.pd_text_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def append_sites(self, tid, beg, n, name):
        nm = name.encode() if isinstance(name, str) else bytes(name)
        got = ctypes.c_uint64()
        self.e._ck(self.e.L.pd_text_append_sites(self.h, int(tid), int(beg), int(n), nm, len(nm), ctypes.byref(got)))
        return int(got.value)

    def append_window_rows(self, tid, w, row_first, n_rows, name):
        nm = name.encode() if isinstance(name, str) else bytes(name)
        got = ctypes.c_uint64()
        self.e._ck(self.e.L.pd_text_append_window_rows(self.h, int(tid), int(w), int(row_first), int(n_rows), nm, len(nm), ctypes.byref(got)))
        return int(got.value)

    def append_bytes(self, data):
        b = np.frombuffer(bytes(data), dtype=np.uint8)
        self.e._ck(self.e.L.pd_text_append_bytes(self.h, _ptr(b) if b.size else None, b.size))

    def parse(self, off, n, chunks, crc_span):
        ch = np.ascontiguousarray(np.asarray(chunks, dtype=np.uint64).reshape(-1, 3))
        cap = int(sum(int(e - s) for s, e, _ in ch.tolist())) + 16
        syms = np.zeros(cap, dtype=np.uint32)
        soff = np.zeros(ch.shape[0] + 1, dtype=np.uint64)
        crc = np.zeros(max(1, ch.shape[0]), dtype=np.uint32)
        self.e._ck(self.e.L.pd_text_parse(self.h, int(off), int(n), _ptr(ch), ch.shape[0], _ptr(syms), cap, _ptr(soff), _ptr(crc), int(crc_span)))
        return [syms[int(soff[k]):int(soff[k + 1])] for k in range(ch.shape[0])], crc[:ch.shape[0]]

    def read(self, off, n):
        buf = np.empty(max(1, int(n)), dtype=np.uint8)
        self.e._ck(self.e.L.pd_text_read(self.h, int(off), int(n), _ptr(buf)))
        return buf[:int(n)].tobytes()

    def release(self, off):
        self.e._ck(self.e.L.pd_text_release(self.h, int(off)))
