"""ctypes binding of the C-ABI (include/zfec_hip.h) of libzfec_hip.so.

This is the binding a ctypes/FFI user of zfec's fec.h would write (see
INTEGRATION.md); tests use it to exercise the C entry points directly and
bench.py uses the batched, stream-ordered extensions with device buffers.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZFEC_HIP_LIB: another build of the library (make asan-py: the host code built
# with AddressSanitizer); the default is the in-tree build next to this file
LIB_PATH = os.environ.get("ZFEC_HIP_LIB") or os.path.join(_HERE, "libzfec_hip.so")

FEC_OK, FEC_EINVAL, FEC_ENODEV, FEC_EHIP, FEC_ENOMEM, FEC_ESINGULAR, FEC_EUNINIT = range(7)
FEC_FLAG_ASYNC = 1
FEC_FLAG_LIBRARY_STREAM = 2
FEC_FLAG_ALL_PRIMARIES = 4
FEC_FLAG_HOST_MEMORY = 8
FEC_FLAG_ROW_PADDING = 16
FEC_FLAG_NO_POPULATE = 32

# (name, restype, argtypes) for every symbol declared in include/zfec_hip.h
_P = ctypes.c_void_p
_SZ = ctypes.c_size_t
_U = ctypes.c_uint
_UP = ctypes.POINTER(ctypes.c_uint)
_PP = ctypes.POINTER(ctypes.c_void_p)
_IP = ctypes.POINTER(ctypes.c_int)
SYMBOLS = [
    ("fec_init", None, []),
    ("fec_new", _P, [ctypes.c_ushort, ctypes.c_ushort]),
    ("fec_free", None, [_P]),
    ("fec_encode", None, [_P, _PP, _PP, _UP, _SZ, _SZ]),
    ("fec_decode", None, [_P, _PP, _PP, _UP, _SZ]),
    ("build_decode_matrix_into_space", None, [_P, _UP, _U, _P]),
    ("_invert_vdm", None, [_P, _U]),
    ("fec_last_status", ctypes.c_int, []),
    ("fec_last_error_message", ctypes.c_char_p, []),
    ("fec_encode_ex", ctypes.c_int, [_P, _PP, _PP, _UP, _SZ, _SZ, _P, _U]),
    ("fec_decode_ex", ctypes.c_int, [_P, _PP, _PP, _UP, _SZ, _P, _U]),
    ("fec_encode_batch", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _SZ, _SZ, _P, _U]),
    ("fec_decode_batch", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _SZ, _P, _U]),
    ("fec_host_alloc", _P, [_SZ]),
    ("fec_host_free", None, [_P]),
    ("fec_device_count", ctypes.c_int, []),
    ("fec_version", ctypes.c_char_p, []),
    ("fec_kernel_name", ctypes.c_char_p, [_U, _U]),
    ("fec_last_kernel_name", ctypes.c_char_p, []),
    ("fec_jit_mode", ctypes.c_int, [ctypes.c_int]),
    ("fec_jit_wait", ctypes.c_int, []),
    ("fec_generic_mode", ctypes.c_int, [ctypes.c_int]),
    ("fec_jit_prepare_encode", ctypes.c_int, [_P, _UP, _SZ]),
    ("fec_jit_prepare_decode", ctypes.c_int, [_P, _UP, _U]),
    ("fec_encode_batch_multi", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _SZ, _SZ, _IP, _SZ, _U]),
    ("fec_decode_batch_multi", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _SZ, _IP, _SZ, _U]),
    ("fec_reload_config", ctypes.c_int, []),
    ("fec_last_wait", ctypes.c_int, []),
    ("fec_run_batch_jobs", ctypes.c_int, [_P, _SZ, _P, _U]),
    ("fec_decode_batch_mixed", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _P, _SZ, _SZ, _P, _U]),
    ("fec_mixed_decode_rows", ctypes.c_int, [_P, _UP, _P]),
    ("fec_verify_batch", ctypes.c_int, [_P, _P, _SZ, _SZ, _UP, _SZ, _SZ, _SZ, _P, _P, _U]),
    ("fec_verify_rows", ctypes.c_int, [_P, _UP, _SZ, _P]),
    ("fec_repair_batch", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _UP, _SZ, _SZ, _P, _SZ, _SZ, _P, _U]),
    ("fec_repair_rows", ctypes.c_int, [_P, _UP, _UP, _SZ, _P]),
    ("fec_locate_batch", ctypes.c_int, [_P, _P, _SZ, _SZ, _UP, _SZ, _SZ, _SZ, _P, _P, _U]),
    ("fec_locate_rows", ctypes.c_int, [_P, _UP, _SZ, _P]),
    ("fec_correct_batch", ctypes.c_int, [_P, _P, _SZ, _SZ, _UP, _SZ, _SZ, _SZ, _P, _P, _U]),
    ("fec_correct_rows", ctypes.c_int, [_P, _UP, _SZ, _P]),
    ("fec_locate2_batch", ctypes.c_int, [_P, _P, _SZ, _SZ, _UP, _SZ, _SZ, _SZ, _P, _P, _U]),
    ("fec_locate2_rows", ctypes.c_int, [_P, _UP, _SZ, _U, _U, _P]),
    ("fec_correct2_batch", ctypes.c_int, [_P, _P, _SZ, _SZ, _UP, _SZ, _SZ, _SZ, _P, _P, _U]),
    ("fec_correct2_rows", ctypes.c_int, [_P, _UP, _SZ, _U, _U, _UP, _P]),
    ("fec_repair_plan_new", ctypes.c_int, [_P, _UP, _UP, _SZ, _SZ, ctypes.c_int, _PP]),
    ("fec_repair_plan_free", None, [_P]),
    ("fec_repair_batch_planned", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _SZ, _SZ, _P, _SZ, _SZ, _P, _U]),
    ("fec_encode_batch_ragged", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _SZ, _SZ, _P, _P, _UP, _SZ, _SZ, _P, _U]),
    ("fec_decode_batch_ragged", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _SZ, _SZ, _P, _P, _UP, _SZ, _P, _U]),
    ("fec_ragged_units", ctypes.c_int, [_P, _SZ, _P]),
    ("fec_verify_batch_ragged", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _UP, _SZ, _SZ, _P, _P, _U]),
    ("fec_locate_batch_ragged", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _UP, _SZ, _SZ, _P, _P, _U]),
    ("fec_repair_batch_ragged", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _SZ, _SZ, _P, _P, _UP, _UP, _SZ, _SZ, _P, _SZ,
                                               _P, _U]),
    ("fec_correct_batch_ragged", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _UP, _SZ, _SZ, _P, _P, _U]),
    ("fec_locate2_batch_ragged", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _UP, _SZ, _SZ, _P, _P, _U]),
    ("fec_correct2_batch_ragged", ctypes.c_int, [_P, _P, _SZ, _SZ, _P, _P, _UP, _SZ, _SZ, _P, _P, _U]),
    ("fec_update_batch", ctypes.c_int, [_P, _P, _P, _SZ, _SZ, _P, _SZ, _SZ, _UP, _SZ, _P, _SZ, _SZ, _SZ, _P, _U]),
    ("fec_update_rows", ctypes.c_int, [_P, _UP, _SZ, _U, _P]),
    ("fec_update_batch_ragged", ctypes.c_int, [_P, _P, _P, _SZ, _SZ, _P, _P, _SZ, _SZ, _P, _P, _UP, _SZ, _P, _SZ, _SZ, _P,
                                               _U]),
]
FEC_LOCATE_CLEAN, FEC_LOCATE_MANY, FEC_LOCATE_UNKNOWN = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD  # fec_locate_batch verdicts
FEC_LOCATE_NONE = 0xFFFFFFFC  # fec_locate2_batch: the second word of a verdict that is no pair
FEC_LOCATE_UNFIT = 0xFFFFFFFB  # fec_locate_batch_ragged: a device-side descriptor that does not fit the arena
LOCATE_UNFIT = -5  # the same as the int32 the Python methods return
FEC_REPAIR_NONE = 0xFFFFFFFF  # a target slot its pattern does not use
FEC_UPDATE_NONE = 0xFFFFFFFF  # fec_update_batch: a slot of `changed` its stripe does not use

JIT_OFF, JIT_AUTO, JIT_FORCE = 0, 1, 2
FEC_JOB_ENCODE, FEC_JOB_DECODE = 0, 1


class FecT(ctypes.Structure):
    """Layout of fec_t (zfec/fec.h:11-15 prefix + priv)."""

    _fields_ = [("magic", ctypes.c_ulong), ("k", ctypes.c_ushort), ("n", ctypes.c_ushort),
                ("enc_matrix", ctypes.POINTER(ctypes.c_ubyte)), ("priv", ctypes.c_void_p)]


_lib = None
# zfec_amd._fec.batch_call: the batched entry points called from C (the ctypes
# conversion of their thirteen arguments is ~2 us of host cost per call).  Only
# with the in-tree library, which the extension links: with ZFEC_HIP_LIB set
# (another build) every call stays on that library through ctypes.
_batch_call = None


def lib():
    global _lib, _batch_call
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libzfec_hip.so is not built (run `make` or __graft_entry__.build())")
        from . import _runtime

        _runtime.preload()
        L = ctypes.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        L.fec_init()
        _lib = L
        if not os.environ.get("ZFEC_HIP_LIB") and not os.environ.get("ZFEC_CAPI_CTYPES"):
            try:
                from . import _fec
            except ImportError:
                _fec = None
            _batch_call = getattr(_fec, "batch_call", None)
    return _lib


class FecError(RuntimeError):
    pass


def check(status):
    if status != FEC_OK:
        raise FecError("zfec-hip status %d: %s" % (status, lib().fec_last_error_message().decode()))


def variant_name(k, r):
    """Kernel variant used for k inputs and r outputs (fec_kernel_name)."""
    return lib().fec_kernel_name(k, r).decode()


def last_kernel_name():
    """Kernel the calling thread launched last (fec_last_kernel_name)."""
    return lib().fec_last_kernel_name().decode()


def jit_mode(mode=-1):
    """Set the bit-sliced JIT mode (JIT_OFF / JIT_AUTO / JIT_FORCE); returns the previous one."""
    return lib().fec_jit_mode(mode)


def generic_mode(mode=-1):
    """Run-time-data bit-sliced kernels for wide-code launches no JIT kernel
    serves: 2 = matapply_bsr where it fits, else matapply_bsg (default);
    1 = matapply_bsg only; 0 = off (table kernels).  Returns the previous mode."""
    return lib().fec_generic_mode(mode)


def jit_wait():
    """Wait for background JIT compiles; number of compiled kernels."""
    return lib().fec_jit_wait()


def reload_config():
    """Re-read the ZFEC_HIP_* environment knobs (read once per process
    otherwise; tests and A/B runs)."""
    check(lib().fec_reload_config())


def last_wait():
    """1 if the calling thread's last synchronous small-object call waited on
    the completion word its kernel wrote, 0 if on hipStreamSynchronize."""
    return lib().fec_last_wait()


def ragged_units(sizes):
    """fec_ragged_units: the exclusive prefix sum of ceil(size / 1024) over
    `sizes`, len(sizes) + 1 ints; the last one is the total."""
    n = len(sizes)
    arr = (ctypes.c_ulonglong * max(1, n))(*[int(x) for x in sizes])
    out = (ctypes.c_ulonglong * (n + 1))()
    check(lib().fec_ragged_units(ctypes.addressof(arr), n, ctypes.addressof(out)))
    return list(out)


def ptr_array(addrs):
    return (ctypes.c_void_p * max(1, len(addrs)))(*addrs)


def uint_array(vals):
    return (ctypes.c_uint * max(1, len(vals)))(*vals)


_UINT_CACHE = {}


def _nums(vals):
    """uint_array(vals), cached per tuple of values: a batched call's block
    numbers are usually the same every call (the ctypes array construction
    is about a microsecond of the per-call host cost)."""
    key = tuple(vals)
    a = _UINT_CACHE.get(key)
    if a is None:
        if len(_UINT_CACHE) > 4096:
            _UINT_CACHE.clear()
        a = _UINT_CACHE[key] = uint_array(key)
    return a


def _uint_table(rows, width, what):
    """((unsigned* argument, keep-alive), nrows, width) of a table of unsigned
    numbers: a sequence of equally long sequences or a 2-D integer numpy array;
    -1 stands for 0xFFFFFFFF.  `width`: the required row length, or None."""
    if hasattr(rows, "ctypes"):
        import numpy as np

        if rows.ndim != 2 or (rows.size and rows.dtype.kind not in "iu") or (width is not None and
                                                                           rows.shape[1] != width):
            raise FecError(what)
        arr = np.ascontiguousarray(rows.astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
        return (ctypes.cast(arr.ctypes.data, _UP) if arr.size else uint_array([]), arr), arr.shape[0], arr.shape[1]
    rows = [tuple(r) for r in rows]
    w = width if width is not None else (len(rows[0]) if rows else 0)
    for r in rows:
        if len(r) != w:
            raise FecError(what)
    return (uint_array([int(x) & 0xFFFFFFFF for r in rows for x in r]), None), len(rows), w


class Code(object):
    """RAII wrapper around fec_t* (fec_new / fec_free)."""

    def __init__(self, k, m):
        self.k, self.m = k, m
        self.ptr = lib().fec_new(k, m)
        if not self.ptr:
            raise FecError("fec_new(%d, %d) failed: %s" % (k, m, lib().fec_last_error_message().decode()))

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.fec_free(self.ptr)
            self.ptr = None

    def enc_matrix(self):
        s = ctypes.cast(self.ptr, ctypes.POINTER(FecT)).contents
        return bytes(s.enc_matrix[: self.k * self.m])

    def jit_prepare_encode(self, block_nums):
        check(lib().fec_jit_prepare_encode(self.ptr, uint_array(block_nums), len(block_nums)))

    def jit_prepare_decode(self, index, flags=0):
        check(lib().fec_jit_prepare_decode(self.ptr, uint_array(index), flags))

    def encode_batch(self, src, sbs, sss, dst, dbs, dss, block_nums, sz, nstripes, stream=0, flags=FEC_FLAG_ASYNC):
        if _batch_call is not None:
            st = _batch_call(0, self.ptr, src, sbs, sss, dst, dbs, dss, block_nums, sz, nstripes, stream or 0, flags)
            if st:
                check(st)
            return
        st = _lib.fec_encode_batch(self.ptr, src, sbs, sss, dst, dbs, dss, _nums(block_nums), len(block_nums), sz,
                                   nstripes, stream or None, flags)
        if st:
            check(st)

    def decode_batch(self, src, sbs, sss, dst, dbs, dss, index, sz, nstripes, stream=0, flags=FEC_FLAG_ASYNC):
        if _batch_call is not None:
            st = _batch_call(1, self.ptr, src, sbs, sss, dst, dbs, dss, index, sz, nstripes, stream or 0, flags)
            if st:
                check(st)
            return
        st = _lib.fec_decode_batch(self.ptr, src, sbs, sss, dst, dbs, dss, _nums(index), sz, nstripes,
                                   stream or None, flags)
        if st:
            check(st)

    def decode_batch_mixed(self, src, sbs, sss, dst, dbs, dss, patterns, pattern_of_ptr, sz, nstripes, stream=0,
                           flags=FEC_FLAG_ASYNC):
        """fec_decode_batch_mixed: `patterns` is a sequence of k-number
        sequences (or a [P, k] integer numpy array); `pattern_of_ptr` is the
        address of nstripes uint32 pattern ids in host or device memory, which
        the caller keeps alive until the call returns."""
        if hasattr(patterns, "ctypes"):
            import numpy as np

            pats = np.ascontiguousarray(patterns, dtype=np.uint32)
            npat = pats.shape[0] if pats.ndim == 2 else 0
            if pats.ndim != 2 or pats.shape[1] != self.k:
                raise FecError("patterns is required to be [npatterns, k = %d]" % self.k)
            arr = ctypes.cast(pats.ctypes.data, _UP) if pats.size else uint_array([])
        else:
            rows = [tuple(p) for p in patterns]
            for p in rows:
                if len(p) != self.k:
                    raise FecError("patterns is required to be [npatterns, k = %d]" % self.k)
            npat = len(rows)
            arr = uint_array([x for p in rows for x in p])
        st = lib().fec_decode_batch_mixed(self.ptr, src, sbs, sss, dst, dbs, dss, arr, npat, pattern_of_ptr or None, sz,
                                          nstripes, stream or None, flags)
        if st:
            check(st)

    def encode_batch_ragged(self, src, src_bytes, sbs, src_offsets_ptr, dst, dst_bytes, dbs, dst_offsets_ptr,
                            sizes_ptr, block_nums, nstripes, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_encode_batch_ragged: the three `_ptr` arguments are the
        addresses of nstripes 8-byte words each, all in host or all in device
        memory, which the caller keeps alive until the call returns."""
        st = lib().fec_encode_batch_ragged(self.ptr, src, src_bytes, sbs, src_offsets_ptr or None, dst, dst_bytes,
                                           dbs, dst_offsets_ptr or None, sizes_ptr or None, _nums(block_nums),
                                           len(block_nums), nstripes, stream or None, flags)
        if st:
            check(st)

    def decode_batch_ragged(self, src, src_bytes, sbs, src_offsets_ptr, dst, dst_bytes, dbs, dst_offsets_ptr,
                            sizes_ptr, index, nstripes, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_decode_batch_ragged: as encode_batch_ragged, with
        decode_batch's index."""
        st = lib().fec_decode_batch_ragged(self.ptr, src, src_bytes, sbs, src_offsets_ptr or None, dst, dst_bytes,
                                           dbs, dst_offsets_ptr or None, sizes_ptr or None, _nums(index), nstripes,
                                           stream or None, flags)
        if st:
            check(st)

    def repair_batch(self, src, sbs, sss, dst, dbs, dss, present, targets, pattern_of_ptr, sz, nstripes, stream=0,
                     flags=FEC_FLAG_ASYNC):
        """fec_repair_batch: `present` is a sequence of k-number sequences (or
        a [P, k] integer numpy array), `targets` one of t-number sequences (or
        [P, t]) whose entries are block numbers or FEC_REPAIR_NONE (-1 is taken
        for it); `pattern_of_ptr` is the address of nstripes uint32 pattern ids
        in host or device memory, which the caller keeps alive until the call
        returns, or 0 (P = 1: every stripe uses pattern 0)."""
        pres, npat, _ = _uint_table(present, self.k, "present is required to be [npatterns, k = %d]" % self.k)
        tgts, ntp, nt = _uint_table(targets, None, "targets is required to be [npatterns, ntargets]")
        if ntp != npat:
            raise FecError("targets is required to hold one row per pattern: %d rows, %d patterns" % (ntp, npat))
        st = lib().fec_repair_batch(self.ptr, src, sbs, sss, dst, dbs, dss, pres[0], tgts[0], nt, npat,
                                    pattern_of_ptr or None, sz, nstripes, stream or None, flags)
        if st:
            check(st)

    def update_batch(self, oldb, newb, ibs, iss, rows, rbs, rss, block_nums, changed_ptr, nchanged, sz, nstripes,
                     stream=0, flags=FEC_FLAG_ASYNC):
        """fec_update_batch: `oldb` is 0 when `newb` holds the deltas;
        `changed_ptr` is the address of nstripes * nchanged uint32 primary
        numbers (FEC_UPDATE_NONE for an unused slot) in host or device memory,
        which the caller keeps alive until the call returns."""
        st = lib().fec_update_batch(self.ptr, oldb or None, newb or None, ibs, iss, rows or None, rbs, rss,
                                    _nums(block_nums), len(block_nums), changed_ptr or None, nchanged, sz, nstripes,
                                    stream or None, flags)
        if st:
            check(st)

    def update_batch_ragged(self, oldb, newb, in_bytes, ibs, in_offsets_ptr, rows, row_bytes, rbs, row_offsets_ptr,
                            sizes_ptr, block_nums, changed_ptr, nchanged, nstripes, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_update_batch_ragged: update_batch over stripes that each have
        their own size.  `oldb` is 0 when `newb` holds the deltas; the three
        `_ptr` descriptor arguments are the addresses of nstripes 8-byte words
        each, all in host or all in device memory, and `changed_ptr` that of
        nstripes * nchanged uint32 primary numbers (FEC_UPDATE_NONE for an
        unused slot) in host or device memory; the caller keeps them alive
        until the call returns."""
        st = lib().fec_update_batch_ragged(self.ptr, oldb or None, newb or None, in_bytes, ibs, in_offsets_ptr or None,
                                           rows or None, row_bytes, rbs, row_offsets_ptr or None, sizes_ptr or None,
                                           _nums(block_nums), len(block_nums), changed_ptr or None, nchanged, nstripes,
                                           stream or None, flags)
        if st:
            check(st)

    def repair_plan(self, present, targets, device=None):
        """fec_repair_plan_new: the patterns of repair_batch (`present` [P, k],
        `targets` [P, t], -1 for FEC_REPAIR_NONE) resolved once into a
        RepairPlan on `device` (None: the current device).  A decode plan is
        targets = 0..k-1 for every pattern."""
        pres, npat, _ = _uint_table(present, self.k, "present is required to be [npatterns, k = %d]" % self.k)
        tgts, ntp, nt = _uint_table(targets, None, "targets is required to be [npatterns, ntargets]")
        if ntp != npat:
            raise FecError("targets is required to hold one row per pattern: %d rows, %d patterns" % (ntp, npat))
        out = ctypes.c_void_p()
        check(lib().fec_repair_plan_new(self.ptr, pres[0], tgts[0], nt, npat, -1 if device is None else int(device),
                                        ctypes.byref(out)))
        return RepairPlan(out.value, self.k, nt, npat)

    def verify_batch(self, src, sbs, sss, block_nums, sz, nstripes, mismatch_ptr, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_verify_batch: slot j of every stripe holds block block_nums[j],
        the first k slots the basis, the rest the checks; `mismatch_ptr` is the
        address of nstripes * ceil((len(block_nums) - k) / 32) uint32 words in
        device or host memory, which the library clears and sets bits in."""
        st = lib().fec_verify_batch(self.ptr, src, sbs, sss, _nums(block_nums), len(block_nums), sz, nstripes,
                                    mismatch_ptr or None, stream or None, flags)
        if st:
            check(st)

    def locate_batch(self, src, sbs, sss, block_nums, sz, nstripes, culprit_ptr, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_locate_batch: the arguments of verify_batch; `culprit_ptr` is the
        address of nstripes uint32 words in device or host memory, each set to
        the corrupt block's slot index or to FEC_LOCATE_CLEAN / _MANY /
        _UNKNOWN."""
        st = lib().fec_locate_batch(self.ptr, src, sbs, sss, _nums(block_nums), len(block_nums), sz, nstripes,
                                    culprit_ptr or None, stream or None, flags)
        if st:
            check(st)

    def verify_batch_ragged(self, src, src_bytes, sbs, src_offsets_ptr, sizes_ptr, block_nums, nstripes, mismatch_ptr,
                            stream=0, flags=FEC_FLAG_ASYNC):
        """fec_verify_batch_ragged: verify_batch over stripes that each have
        their own size; the two `_ptr` descriptor arguments are the addresses
        of nstripes 8-byte words each, both in host or both in device memory,
        which the caller keeps alive until the call returns."""
        st = lib().fec_verify_batch_ragged(self.ptr, src, src_bytes, sbs, src_offsets_ptr or None, sizes_ptr or None,
                                           _nums(block_nums), len(block_nums), nstripes, mismatch_ptr or None,
                                           stream or None, flags)
        if st:
            check(st)

    def locate_batch_ragged(self, src, src_bytes, sbs, src_offsets_ptr, sizes_ptr, block_nums, nstripes, culprit_ptr,
                            stream=0, flags=FEC_FLAG_ASYNC):
        """fec_locate_batch_ragged: as verify_batch_ragged, with locate_batch's
        verdict words (and FEC_LOCATE_UNFIT for a device-side descriptor that
        does not fit)."""
        st = lib().fec_locate_batch_ragged(self.ptr, src, src_bytes, sbs, src_offsets_ptr or None, sizes_ptr or None,
                                           _nums(block_nums), len(block_nums), nstripes, culprit_ptr or None,
                                           stream or None, flags)
        if st:
            check(st)

    def repair_batch_ragged(self, src, src_bytes, sbs, src_offsets_ptr, dst, dst_bytes, dbs, dst_offsets_ptr,
                            sizes_ptr, present, targets, pattern_of_ptr, nstripes, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_repair_batch_ragged: the arena arguments of encode_batch_ragged
        (three `_ptr` descriptor arrays of nstripes 8-byte words, all in host
        or all in device memory) and the pattern arguments of repair_batch
        (`present` [P, k], `targets` [P, t] with -1 for FEC_REPAIR_NONE,
        `pattern_of_ptr` the address of nstripes uint32 ids in host or device
        memory, or 0 with P = 1)."""
        pres, npat, _ = _uint_table(present, self.k, "present is required to be [npatterns, k = %d]" % self.k)
        tgts, ntp, nt = _uint_table(targets, None, "targets is required to be [npatterns, ntargets]")
        if ntp != npat:
            raise FecError("targets is required to hold one row per pattern: %d rows, %d patterns" % (ntp, npat))
        st = lib().fec_repair_batch_ragged(self.ptr, src, src_bytes, sbs, src_offsets_ptr or None, dst, dst_bytes, dbs,
                                           dst_offsets_ptr or None, sizes_ptr or None, pres[0], tgts[0], nt, npat,
                                           pattern_of_ptr or None, nstripes, stream or None, flags)
        if st:
            check(st)

    def correct_batch_ragged(self, blocks, nbytes, bs, offsets_ptr, sizes_ptr, block_nums, nstripes, culprit_ptr,
                             stream=0, flags=FEC_FLAG_ASYNC):
        """fec_correct_batch_ragged: the arguments of locate_batch_ragged,
        `blocks` writable: the verdicts go to `culprit_ptr` as there, and the
        slot a verdict names is rewritten in place."""
        st = lib().fec_correct_batch_ragged(self.ptr, blocks, nbytes, bs, offsets_ptr or None, sizes_ptr or None,
                                            _nums(block_nums), len(block_nums), nstripes, culprit_ptr or None,
                                            stream or None, flags)
        if st:
            check(st)

    def correct_batch(self, blocks, bs, ss, block_nums, sz, nstripes, culprit_ptr, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_correct_batch: the arguments of locate_batch, `blocks` writable.
        The verdicts go to `culprit_ptr` as there, and the slot a verdict names
        is rewritten in place from k other slots of its stripe."""
        st = lib().fec_correct_batch(self.ptr, blocks, bs, ss, _nums(block_nums), len(block_nums), sz, nstripes,
                                     culprit_ptr or None, stream or None, flags)
        if st:
            check(st)

    def locate2_batch(self, src, sbs, sss, block_nums, sz, nstripes, culprit_ptr, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_locate2_batch: the arguments of locate_batch; `culprit_ptr` is
        the address of 2 * nstripes uint32 words in device or host memory, two
        planes: word s and word nstripes + s are stripe s's verdict, a pair of
        slots (a, b) or locate_batch's verdict and FEC_LOCATE_NONE."""
        st = lib().fec_locate2_batch(self.ptr, src, sbs, sss, _nums(block_nums), len(block_nums), sz, nstripes,
                                     culprit_ptr or None, stream or None, flags)
        if st:
            check(st)

    def correct2_batch(self, blocks, bs, ss, block_nums, sz, nstripes, culprit_ptr, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_correct2_batch: the arguments of locate2_batch, `blocks`
        writable.  The slot or the two slots a verdict names are rewritten in
        place from k other slots of their stripe."""
        st = lib().fec_correct2_batch(self.ptr, blocks, bs, ss, _nums(block_nums), len(block_nums), sz, nstripes,
                                      culprit_ptr or None, stream or None, flags)
        if st:
            check(st)

    def locate2_batch_ragged(self, src, src_bytes, sbs, src_offsets_ptr, sizes_ptr, block_nums, nstripes, culprit_ptr,
                             stream=0, flags=FEC_FLAG_ASYNC):
        """fec_locate2_batch_ragged: the arguments of locate_batch_ragged;
        `culprit_ptr` is the address of 2 * nstripes uint32 words in device or
        host memory, the two planes of locate2_batch (FEC_LOCATE_UNFIT in
        plane 0 for a device-side descriptor that does not fit)."""
        st = lib().fec_locate2_batch_ragged(self.ptr, src, src_bytes, sbs, src_offsets_ptr or None, sizes_ptr or None,
                                            _nums(block_nums), len(block_nums), nstripes, culprit_ptr or None,
                                            stream or None, flags)
        if st:
            check(st)

    def correct2_batch_ragged(self, blocks, nbytes, bs, offsets_ptr, sizes_ptr, block_nums, nstripes, culprit_ptr,
                              stream=0, flags=FEC_FLAG_ASYNC):
        """fec_correct2_batch_ragged: the arguments of locate2_batch_ragged,
        `blocks` writable.  The slot or the two slots a verdict names are
        rewritten in place, sizes[s] bytes each."""
        st = lib().fec_correct2_batch_ragged(self.ptr, blocks, nbytes, bs, offsets_ptr or None, sizes_ptr or None,
                                             _nums(block_nums), len(block_nums), nstripes, culprit_ptr or None,
                                             stream or None, flags)
        if st:
            check(st)

    def encode_batch_multi(self, src, sbs, sss, dst, dbs, dss, block_nums, sz, nstripes, devices, flags=0):
        """fec_encode_batch_multi: the stripes split over `devices` (host memory)."""
        devs = (ctypes.c_int * max(1, len(devices)))(*devices)
        check(lib().fec_encode_batch_multi(self.ptr, src, sbs, sss, dst, dbs, dss, uint_array(block_nums),
                                           len(block_nums), sz, nstripes, devs, len(devices), flags))

    def decode_batch_multi(self, src, sbs, sss, dst, dbs, dss, index, sz, nstripes, devices, flags=0):
        """fec_decode_batch_multi: the stripes split over `devices` (host memory)."""
        devs = (ctypes.c_int * max(1, len(devices)))(*devices)
        check(lib().fec_decode_batch_multi(self.ptr, src, sbs, sss, dst, dbs, dss, uint_array(index), sz, nstripes,
                                           devs, len(devices), flags))

    def encode_ptrs(self, in_addrs, out_addrs, block_nums, sz, stream=0, flags=FEC_FLAG_ASYNC):
        check(lib().fec_encode_ex(self.ptr, ptr_array(in_addrs), ptr_array(out_addrs), uint_array(block_nums),
                                  len(block_nums), sz, stream or None, flags))

    def decode_ptrs(self, in_addrs, out_addrs, index, sz, stream=0, flags=FEC_FLAG_ASYNC):
        check(lib().fec_decode_ex(self.ptr, ptr_array(in_addrs), ptr_array(out_addrs), uint_array(index),
                                  sz, stream or None, flags))


class RepairPlan(object):
    """A fec_repair_plan_t*: immutable, usable from any thread on any stream
    until close() (fec_repair_plan_free).  The caller keeps it alive as long
    as calls, and graphs captured from them, are in flight."""

    def __init__(self, ptr, k, ntargets, npatterns):
        self.ptr, self.k, self.ntargets, self.npatterns = ptr, k, ntargets, npatterns

    def repair_batch(self, src, sbs, sss, dst, dbs, dss, pattern_of_ptr, sz, nstripes, stream=0, flags=FEC_FLAG_ASYNC):
        """fec_repair_batch_planned: Code.repair_batch's arguments without the
        patterns; `pattern_of_ptr` is the address of nstripes uint32 pattern
        ids in host or device memory."""
        if not self.ptr:
            raise FecError("the repair plan is closed")
        st = lib().fec_repair_batch_planned(self.ptr, src, sbs, sss, dst, dbs, dss, pattern_of_ptr or None, sz, nstripes,
                                            stream or None, flags)
        if st:
            check(st)

    def close(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.fec_repair_plan_free(self.ptr)
        self.ptr = None

    __del__ = close


def mixed_decode_rows(code, pattern):
    """fec_mixed_decode_rows: the k*k bytes (row-major) of the matrix
    fec_decode_batch_mixed applies for `pattern` (k block numbers, any slot
    order); row i yields primary i.  Host only."""
    pattern = list(pattern)
    if len(pattern) != code.k:
        raise FecError("pattern is required to hold k = %d block numbers" % code.k)
    rows = (ctypes.c_ubyte * (code.k * code.k))()
    check(lib().fec_mixed_decode_rows(code.ptr, uint_array(pattern), ctypes.cast(rows, _P)))
    return bytes(rows)


def verify_rows(code, block_nums):
    """fec_verify_rows: the c*k bytes (row-major, c = len(block_nums) - k) of
    the matrix fec_verify_batch applies for `block_nums`; row i yields the
    block of slot k + i from the k basis slots.  Host only."""
    nums = list(block_nums)
    rows = (ctypes.c_ubyte * max(1, (len(nums) - code.k) * code.k))()
    check(lib().fec_verify_rows(code.ptr, uint_array(nums), len(nums), ctypes.cast(rows, _P)))
    return bytes(rows)


def locate_rows(code, block_nums):
    """fec_locate_rows: the (c-1)*k bytes (row-major, c = len(block_nums) - k)
    of the matrix Q fec_locate_batch tests with, Q[i][j] = P[i][j] / P[0][j]
    for i = 1..c-1; empty for c == 1.  Host only."""
    nums = list(block_nums)
    n = max(0, (len(nums) - code.k - 1) * code.k)
    rows = (ctypes.c_ubyte * max(1, n))()
    check(lib().fec_locate_rows(code.ptr, uint_array(nums), len(nums), ctypes.cast(rows, _P)))
    return bytes(rows)[:n]


def correct_rows(code, block_nums):
    """fec_correct_rows: the nb*k bytes (row-major, nb = len(block_nums)) of
    the matrix fec_correct_batch applies; row h rebuilds slot h from slots
    0..k-1, slot k (check 0) standing in for slot h when h < k.  Host only."""
    nums = list(block_nums)
    n = len(nums) * code.k
    rows = (ctypes.c_ubyte * max(1, n))()
    check(lib().fec_correct_rows(code.ptr, uint_array(nums), len(nums), ctypes.cast(rows, _P)))
    return bytes(rows)[:n]


def locate2_rows(code, block_nums, a, b):
    """fec_locate2_rows: the (c-2)*c bytes (row-major, c = len(block_nums) - k)
    of a matrix N of rank c - 2 that annihilates columns a and b of [P | I]: a
    syndrome vector lies in their span iff N maps it to zero.  Host only."""
    nums = list(block_nums)
    c = len(nums) - code.k
    n = max(0, (c - 2) * c)
    rows = (ctypes.c_ubyte * max(1, n))()
    check(lib().fec_locate2_rows(code.ptr, uint_array(nums), len(nums), a, b, ctypes.cast(rows, _P)))
    return bytes(rows)[:n]


def correct2_rows(code, block_nums, a, b):
    """fec_correct2_rows: (sources, rows): the k lowest slots outside {a, b}
    and the 2*k bytes (row-major) that yield slot a (row 0) and slot b (row 1)
    from them.  Host only."""
    nums = list(block_nums)
    sources = (ctypes.c_uint * code.k)()
    rows = (ctypes.c_ubyte * (2 * code.k))()
    check(lib().fec_correct2_rows(code.ptr, uint_array(nums), len(nums), a, b, sources, ctypes.cast(rows, _P)))
    return list(sources), bytes(rows)


def repair_rows(code, present, targets):
    """fec_repair_rows: the t*k bytes (row-major, t = len(targets)) of the
    matrix fec_repair_batch applies for one pattern; row i yields block
    targets[i] from the k slots holding `present`, a FEC_REPAIR_NONE (or -1)
    row is all zeros.  Host only."""
    present = list(present)
    if len(present) != code.k:
        raise FecError("present is required to hold k = %d block numbers" % code.k)
    tg = [int(x) & 0xFFFFFFFF for x in targets]
    rows = (ctypes.c_ubyte * max(1, len(tg) * code.k))()
    check(lib().fec_repair_rows(code.ptr, uint_array(present), uint_array(tg), len(tg), ctypes.cast(rows, _P)))
    return bytes(rows)[:len(tg) * code.k]


def update_rows(code, block_nums, changed_block):
    """fec_update_rows: the len(block_nums) coefficients E[block_nums[i]][changed_block]
    fec_update_batch multiplies the delta of primary `changed_block` by."""
    nums = list(block_nums)
    coefs = (ctypes.c_ubyte * max(1, len(nums)))()
    check(lib().fec_update_rows(code.ptr, uint_array(nums), len(nums), changed_block, ctypes.cast(coefs, _P)))
    return bytes(coefs[: len(nums)])


class BatchJob(ctypes.Structure):
    """fec_batch_job (include/zfec_hip.h)."""

    _fields_ = [("code", _P), ("kind", _U), ("flags", _U), ("src", _P), ("src_block_stride", _SZ),
                ("src_stripe_stride", _SZ), ("dst", _P), ("dst_block_stride", _SZ), ("dst_stripe_stride", _SZ),
                ("nums", _UP), ("num_nums", _SZ), ("sz", _SZ), ("nstripes", _SZ)]


def encode_job(code, src, sbs, sss, dst, dbs, dss, block_nums, sz, nstripes, flags=0):
    """One fec_run_batch_jobs job: Code.encode_batch's arguments."""
    return (code, FEC_JOB_ENCODE, flags, src, sbs, sss, dst, dbs, dss, tuple(block_nums), sz, nstripes)


def decode_job(code, src, sbs, sss, dst, dbs, dss, index, sz, nstripes, flags=0):
    """One fec_run_batch_jobs job: Code.decode_batch's arguments."""
    return (code, FEC_JOB_DECODE, flags, src, sbs, sss, dst, dbs, dss, tuple(index), sz, nstripes)


class BatchJobs(object):
    """A fec_run_batch_jobs call built once (the ctypes job array and block
    number arrays) and run any number of times."""

    def __init__(self, jobs):
        lib()
        self._codes = [j[0] for j in jobs]  # keep the fec_t objects alive
        self._nums = [uint_array(j[9]) for j in jobs]
        self.n = len(jobs)
        self._arr = (BatchJob * max(1, self.n))()
        for i, (code, kind, flags, src, sbs, sss, dst, dbs, dss, nums, sz, ns) in enumerate(jobs):
            self._arr[i] = BatchJob(code.ptr, kind, flags, src, sbs, sss, dst, dbs, dss,
                                    ctypes.cast(self._nums[i], _UP), len(nums), sz, ns)

    def run(self, stream=0, flags=FEC_FLAG_ASYNC):
        st = _lib.fec_run_batch_jobs(self._arr, self.n, stream or None, flags)
        if st:
            check(st)


def run_batch_jobs(jobs, stream=0, flags=FEC_FLAG_ASYNC):
    """fec_run_batch_jobs over encode_job / decode_job tuples."""
    BatchJobs(jobs).run(stream, flags)
