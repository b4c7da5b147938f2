"""zfec_amd -- zfec's erasure-coding API on AMD MI355X (gfx950).

Drop-in for the reference's Python surface (/root/reference/zfec/__init__.py:12,
zfec/_fecmodule.c): ``Encoder(k, m).encode(inblocks, desired_blocks_nums=None)``,
``Decoder(k, m).decode(blocks, blocknums)``, ``Error``, ``easyfec``.

Bytes-like blocks (bytes, bytearray, memoryview, C-contiguous numpy arrays)
are staged to the GPU and the results come back as ``bytes``, exactly as the
reference returns them.  Device-resident blocks (torch tensors on a ROCm
device) stay on the device: the work is enqueued on the tensor's current
stream and the results are new device tensors.  All GF(2^8) arithmetic runs
in the HIP kernels of libzfec_hip.so; there is no CPU fallback -- importing
fails if the extension is not built, and encode/decode raise ``Error`` when no
GPU is visible.
"""
from . import _runtime

_runtime.preload()  # must precede loading libzfec_hip.so (see _runtime.py)

from . import _fec  # noqa: E402
from ._fec import Error, device_count, test_from_agl, version

__version__ = "0.1.0"

__all__ = ["Encoder", "Decoder", "RepairPlan", "Error", "easyfec", "filefec", "cmdline_zfec", "cmdline_zunfec", "test_from_agl",
           "device_count", "version", "reuse_host_memory", "LOCATE_CLEAN", "LOCATE_MANY", "LOCATE_UNKNOWN",
           "LOCATE_NONE", "LOCATE_UNFIT"]

# Decoder.locate_batch verdicts that are not a slot: FEC_LOCATE_CLEAN / _MANY /
# _UNKNOWN (include/zfec_hip.h) read as int32
LOCATE_CLEAN, LOCATE_MANY, LOCATE_UNKNOWN = -1, -2, -3
# Decoder.locate2_batch: the second word of a verdict that is no pair (FEC_LOCATE_NONE as int32)
LOCATE_NONE = -4
# Decoder.locate_ragged: a device-side descriptor that does not fit the data (FEC_LOCATE_UNFIT as int32)
LOCATE_UNFIT = -5


def _is_device_tensor(x):
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def _byte_view(t):
    import torch

    if not t.is_contiguous():
        raise Error("Precondition violation: Input blocks are required to be C-contiguous.")
    return t.reshape(-1) if t.dtype == torch.uint8 else t.reshape(-1).view(torch.uint8)


def _stream_handle(device):
    import torch

    return torch.cuda.current_stream(device).cuda_stream


def _device_blocks(blocks, k):
    for b in blocks:
        if not _is_device_tensor(b):
            raise Error("Precondition violation: blocks are required to be all device tensors or all host buffers")
    bl = [_byte_view(b) for b in blocks]
    if len(bl) != k:
        raise Error(
            "Precondition violation: Wrong length -- first argument (the sequence of input blocks) is required to "
            "contain exactly k blocks.  len(first): %d, k: %d" % (len(bl), k)
        )
    sz = bl[0].numel() if bl else 0
    dev = bl[0].device if bl else None
    for b in bl:
        if b.numel() != sz:
            raise Error(
                "Precondition violation: Input blocks are required to be all the same length.  length of one block "
                "was: %d, length of another block was: %d" % (sz, b.numel())
            )
        if b.device != dev:
            raise Error("Precondition violation: device blocks are required to be on one device")
    return bl, sz, dev


def _is_host_array(x):
    return type(x).__module__ == "numpy" and hasattr(x, "ctypes")


def _batch_view(blocks, nblocks, what):
    """Check a [nstripes, nblocks, sz] uint8 array for the batched entry points:
    a device tensor, or a host numpy array (pageable memory; the library stages
    it through pinned slots, fec_abi.cpp run_batch_staged).  Any strides with
    unit stride along sz, so a transposed block-major [nblocks, nstripes, sz]
    array passes as is (fec_encode_batch runs it as one long stripe).
    Returns (nstripes, sz, block stride, stripe stride, data pointer)."""
    if _is_host_array(blocks):
        import numpy as np

        if blocks.dtype != np.uint8 or blocks.ndim != 3:
            raise Error("Precondition violation: %s is required to be a uint8 array [nstripes, %d, sz]"
                        % (what, nblocks))
        ns, nb, sz = blocks.shape
        strides = blocks.strides
        ptr = blocks.ctypes.data
    else:
        import torch

        if not _is_device_tensor(blocks) or blocks.dtype != torch.uint8 or blocks.dim() != 3:
            raise Error("Precondition violation: %s is required to be a uint8 device tensor or numpy array "
                        "[nstripes, %d, sz]" % (what, nblocks))
        ns, nb, sz = blocks.shape
        strides = (blocks.stride(0), blocks.stride(1), blocks.stride(2))
        ptr = blocks.data_ptr()
    if nb != nblocks:
        raise Error("Precondition violation: %s is required to hold %d blocks per stripe, not %d" % (what, nblocks, nb))
    if sz > 1 and strides[2] != 1:
        raise Error("Precondition violation: %s blocks are required to be contiguous along sz" % what)
    if min(strides[0], strides[1]) < 0:
        raise Error("Precondition violation: %s is required to have non-negative strides" % what)
    return ns, sz, strides[1], strides[0], ptr


def _batch_out(like, like_block_major, ns, nb, sz):
    """Output [ns, nb, sz] where `like` lives (device tensor or numpy array):
    block-major storage when the input was."""
    shape = (nb, ns, sz) if like_block_major else (ns, nb, sz)
    if _is_host_array(like):
        import numpy as np

        out = np.empty(shape, dtype=np.uint8)
        return out.transpose(1, 0, 2) if like_block_major else out
    import torch

    out = torch.empty(shape, dtype=torch.uint8, device=like.device)
    return out.transpose(0, 1) if like_block_major else out


def _batch_strides(out):
    if _is_host_array(out):
        return out.ctypes.data, out.strides[1], out.strides[0]
    return out.data_ptr(), out.stride(1), out.stride(0)


def _batch_call_args(blocks):
    """stream / flags of a batched call: a device tensor's work is enqueued on
    its current stream; host arrays are synchronous."""
    from . import capi

    if _is_host_array(blocks):
        return 0, capi.FEC_FLAG_LIBRARY_STREAM
    return _stream_handle(blocks.device), capi.FEC_FLAG_ASYNC


class _as_error(object):
    """Library failures of the batched entry points (capi.FecError: no GPU,
    cross-device tensors, ...) surface as zfec_amd.Error like every other
    failure of this API."""

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        from . import capi

        if et is not None and issubclass(et, capi.FecError):
            raise Error(str(ev)) from ev
        return False


def _devices_arg(blocks, devices):
    """None, or the list of devices a host-array batch is split over
    ("all": every visible GPU).  Device tensors stay on their own device."""
    if devices is None:
        return None
    if isinstance(devices, str):
        if devices != "all":
            raise Error("Precondition violation: devices is required to be a list of device indices or 'all'")
        devices = list(range(device_count()))
    devs = [int(d) for d in devices]
    if not devs:
        raise Error("Precondition violation: devices is required to list at least one device")
    if not _is_host_array(blocks):
        if devs != [blocks.device.index if blocks.device.index is not None else 0]:
            raise Error("Precondition violation: a device tensor batch runs on its own device; devices= splits host "
                        "(numpy) batches over several GPUs")
        return None
    return devs


def _ragged_words(x, what):
    """One descriptor array of a ragged call as a contiguous 1-D int64 torch
    tensor: a tensor is checked, a host sequence of ints becomes a CPU tensor."""
    import torch

    if isinstance(x, torch.Tensor):
        if x.dtype != torch.int64 or x.dim() != 1:
            raise Error("Precondition violation: %s is required to be a 1-D int64 tensor or a sequence of ints" % what)
        return x.contiguous()
    try:
        vals = list(x)
    except TypeError:
        raise Error("Precondition violation: %s is required to be a 1-D int64 tensor or a sequence of ints" % what)
    for v in vals:
        if not isinstance(v, int) or isinstance(v, bool):
            raise Error("Precondition violation: %s is required to be a 1-D int64 tensor or a sequence of ints" % what)
        if v < 0 or v >= 2**63:
            raise Error("Precondition violation: %s is required to hold sizes and offsets in [0, 2^63), but one was %d"
                        % (what, v))
    return torch.tensor(vals, dtype=torch.int64)


def _ragged_call(coder, fn, data, sizes, offsets, out, out_offsets, nums, r):
    """The arguments of Encoder.encode_ragged / Decoder.decode_ragged checked
    and completed, then capi.Code.<fn> (or fn itself, a callable that takes
    that method's arguments: Decoder.repair_ragged); returns (out, out_offsets)."""
    import torch

    k = coder.k
    for t, what in ((data, "data"), (out, "out")):
        if t is None and what == "out":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
            raise Error("Precondition violation: %s is required to be a 1-D contiguous uint8 device tensor" % what)
    arrays = [("sizes", _ragged_words(sizes, "sizes"))]
    if offsets is not None:
        arrays.append(("offsets", _ragged_words(offsets, "offsets")))
    if out_offsets is not None:
        arrays.append(("out_offsets", _ragged_words(out_offsets, "out_offsets")))
    sizes = arrays[0][1]
    ns = sizes.numel()
    for what, a in arrays[1:]:
        if a.numel() != ns:
            raise Error("Precondition violation: %s is required to hold one word per stripe: %d, not %d"
                        % (what, ns, a.numel()))
    for what, a in arrays[1:]:
        if a.device != sizes.device:
            raise Error("Precondition violation: sizes, offsets and out_offsets are required to be all on the data's "
                        "device or all on the CPU, but sizes is on %s and %s on %s" % (sizes.device, what, a.device))
    if sizes.is_cuda and sizes.device != data.device:
        raise Error("Precondition violation: sizes, offsets and out_offsets are required to be all on the data's "
                    "device or all on the CPU, but sizes is on %s and data on %s" % (sizes.device, data.device))
    if not sizes.is_cuda:
        for what, a in arrays:
            if ns and int(a.min()) < 0:
                raise Error("Precondition violation: %s is required to hold sizes and offsets in [0, 2^63), but one "
                            "was %d" % (what, int(a.min())))
    if not _is_device_tensor(data) or (out is not None and (not _is_device_tensor(out) or out.device != data.device)):
        raise Error("Precondition violation: data and out are required to be uint8 tensors on one GPU")
    # the packed object-major layout: stripe after stripe, a stripe's blocks back to back
    if offsets is None or out_offsets is None:
        start = torch.cumsum(sizes, 0) - sizes
    offsets = k * start if offsets is None else dict(arrays)["offsets"]
    out_offsets = r * start if out_offsets is None else dict(arrays)["out_offsets"]
    if out is None:
        out = torch.empty(r * int(sizes.sum()) if ns else 0, dtype=torch.uint8, device=data.device)
    if ns and r and data.numel() and out.numel():
        with torch.cuda.device(data.device), _as_error():
            call = fn if callable(fn) else getattr(_capi_code(coder), fn)
            call(data.data_ptr(), data.numel(), 0, offsets.data_ptr(), out.data_ptr(), out.numel(), 0,
                 out_offsets.data_ptr(), sizes.data_ptr(), nums, ns, stream=_stream_handle(data.device))
    return out, out_offsets


def _update_nums(blocknums, k, m, what):
    """The block numbers of the stored rows of an update (default k..m-1):
    distinct ints in [0, m-1]."""
    import numpy as np

    nums = list(range(k, m)) if blocknums is None else list(blocknums)
    for x in nums:
        if not isinstance(x, (int, np.integer)) or isinstance(x, bool) or x < 0 or x >= m:
            raise Error("Precondition violation: %s block nums are required to be in [0, m-1] = "
                        "[0, %d], but one was %r" % (what, m - 1, x))
    nums = [int(x) for x in nums]
    if len(set(nums)) != len(nums):
        raise Error("Precondition violation: %s block nums are required to be distinct, but got %r" % (what, nums))
    return nums


def _update_changed(changed, ns, k, what):
    """The `changed` argument of Encoder.update_batch / update_ragged checked:
    returns (host numbers as a numpy table or None, the device tensor or None,
    slots per stripe)."""
    import numpy as np

    # changed: host numbers as a numpy table, device numbers as they are
    ch = ch_dev = None
    if hasattr(changed, "data_ptr"):
        if changed.dtype.is_floating_point or str(changed.dtype) == "torch.bool":
            raise Error("Precondition violation: changed is required to be an integer array [nstripes] or "
                        "[nstripes, c]")
        if changed.is_cuda:
            ch_dev = changed
            shape = tuple(changed.shape)
        else:
            changed = changed.numpy()
    if ch_dev is None:
        ch = np.asarray(changed)
        if ch.size and ch.dtype.kind not in "iu":
            raise Error("Precondition violation: changed is required to be an integer array [nstripes] or "
                        "[nstripes, c]")
        shape = ch.shape
    if len(shape) not in (1, 2) or shape[0] != ns:
        raise Error("Precondition violation: changed is required to be an integer array [nstripes] or "
                    "[nstripes, c] with nstripes = %d, not %r" % (ns, tuple(shape)))
    c = 1 if len(shape) == 1 else shape[1]
    if c < 1 or c > 4:
        raise Error("Precondition violation: %s takes between 1 and 4 changed blocks per stripe, not %d" % (what, c))
    if ch_dev is None and ch.size and (ch.min() < -1 or ch.max() >= k):
        bad = ch[(ch < -1) | (ch >= k)].reshape(-1)[0]
        raise Error("Precondition violation: changed block nums are required to be primaries in [0, k-1] = "
                    "[0, %d] or -1 (none), but one was %d" % (k - 1, bad))
    return ch, ch_dev, c


def _update_words(ch, ch_dev, k):
    """The uint32 words of checked `changed` numbers: (keep-alive, address)."""
    import numpy as np
    import torch

    if ch_dev is not None:
        # whatever is not a primary becomes -1 (the bits of FEC_UPDATE_NONE) before the
        # narrowing, so that an int64 number like 2^32 + j cannot wrap into the primary j
        wide = ch_dev.to(torch.int64)
        words = torch.where((wide < 0) | (wide >= k), torch.full_like(wide, -1), wide).to(torch.int32).contiguous()
        return words, words.data_ptr()
    words = np.ascontiguousarray(ch.astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)
    return words, words.ctypes.data


def _capi_code(coder):
    code = getattr(coder, "_batch_code", None)
    if code is None:
        from . import capi

        with _as_error():
            code = coder._batch_code = capi.Code(coder.k, coder.m)
    return code


class RepairPlan(object):
    """The erasure patterns of a store resolved once (fec_repair_plan_new): the
    per-pattern matrices are inverted and their kernel tables uploaded at
    creation, and every later call only names each stripe's pattern.  Made by
    Decoder.repair_plan / Decoder.decode_plan; immutable; close() frees it
    (calls in flight, and graphs captured from them, must have finished).

    patterns [P, k] and targets [P, t] are numpy arrays (-1: none); npatterns
    is P."""

    def __init__(self, coder, patterns, targets, decode):
        import numpy as np

        k, m = coder.k, coder.m
        self.k, self.m = k, m
        self.patterns, self.targets = patterns, targets
        self.npatterns, self.ntargets = patterns.shape[0], targets.shape[1]
        self._decode = decode
        with _as_error():
            self._plan = _capi_code(coder).repair_plan(np.ascontiguousarray(patterns, dtype=np.int64),
                                                       np.ascontiguousarray(targets, dtype=np.int64))
        self._coder = coder  # keeps the code alive

    def close(self):
        """Free the plan; harmless when repeated."""
        plan, self._plan = getattr(self, "_plan", None), None
        if plan is not None:
            plan.close()

    def _ids(self, pattern_of, ns, device):
        """(pointer, keep-alive) of nstripes uint32 ids from a 1-D integer list,
        numpy array or torch tensor; a device tensor stays on the device."""
        import numpy as np

        if hasattr(pattern_of, "data_ptr"):
            import torch

            if pattern_of.dim() != 1 or pattern_of.dtype.is_floating_point:
                raise Error("Precondition violation: pattern_of is required to be a 1-D integer array")
            if pattern_of.shape[0] != ns:
                raise Error("Precondition violation: pattern_of is required to hold nstripes = %d ids, not %d"
                            % (ns, pattern_of.shape[0]))
            if pattern_of.is_cuda:
                if pattern_of.device != device:
                    raise Error("Precondition violation: device pattern_of ids are required to be on the blocks' "
                                "device")
                ids = pattern_of.to(torch.int32).contiguous()  # non-negative ids: the bits of uint32
                return ids.data_ptr(), ids
            host = pattern_of.numpy()
        else:
            host = np.asarray(pattern_of)
            if host.ndim != 1 or (host.size and host.dtype.kind not in "iu"):
                raise Error("Precondition violation: pattern_of is required to be a 1-D integer array")
            if host.shape[0] != ns:
                raise Error("Precondition violation: pattern_of is required to hold nstripes = %d ids, not %d"
                            % (ns, host.shape[0]))
        if host.size and (host.min() < 0 or host.max() >= self.npatterns):
            raise Error("Precondition violation: pattern_of ids are required to be in [0, %d]" % (self.npatterns - 1))
        ids = np.ascontiguousarray(host, dtype=np.uint32)
        return ids.ctypes.data, ids

    def repair_batch(self, blocks, pattern_of, out=None):
        """Decoder.repair_batch with the plan's patterns: blocks is a uint8
        device tensor [nstripes, k, sz], pattern_of a 1-D integer list, numpy
        array or torch tensor (host or device) naming each stripe's pattern.
        Returns [nstripes, t, sz] under Decoder.repair_batch's rules: a new
        tensor (block-major when the input was; rows of -1 targets
        unspecified), or `out` with those rows untouched."""
        k, t = self.k, self.ntargets
        if self._plan is None:
            raise Error("Precondition violation: the repair plan is closed")
        if _is_host_array(blocks):
            raise Error("Precondition violation: repair_batch takes a device tensor; host (numpy) blocks are not "
                        "staged by this call")
        is_tensor = type(blocks).__module__.startswith("torch") and hasattr(blocks, "data_ptr")
        if not is_tensor or str(blocks.dtype) != "torch.uint8" or blocks.dim() != 3:
            raise Error("Precondition violation: blocks is required to be a uint8 device tensor [nstripes, %d, sz]" % k)
        if blocks.shape[1] != k:
            raise Error("Precondition violation: blocks is required to hold %d blocks per stripe, not %d"
                        % (k, blocks.shape[1]))
        ns, sz = blocks.shape[0], blocks.shape[2]
        ids_ptr, ids = self._ids(pattern_of, ns, blocks.device)
        if out is not None:
            out_ok = type(out).__module__.startswith("torch") and hasattr(out, "data_ptr")
            if not out_ok or str(out.dtype) != "torch.uint8" or tuple(out.shape) != (ns, t, sz):
                raise Error("Precondition violation: out is required to be a uint8 tensor [nstripes, t, sz] = "
                            "[%d, %d, %d]" % (ns, t, sz))
            if out.device != blocks.device:
                raise Error("Precondition violation: out is required to be on the blocks' device")
            if (sz > 1 and out.stride(2) != 1) or min(out.stride(0), out.stride(1)) < 0:
                raise Error("Precondition violation: out rows are required to be contiguous along sz")
        if not blocks.is_cuda:
            raise Error("Precondition violation: blocks is required to be a uint8 device tensor [nstripes, %d, sz], "
                        "not a host tensor" % k)
        ns, sz, sbs, sss, ptr = _batch_view(blocks, k, "blocks")
        if out is None:
            out = _batch_out(blocks, sss < sbs, ns, t, sz)
        if ns and sz:
            optr, obs, oss = _batch_strides(out)
            stream, flags = _batch_call_args(blocks)
            # `ids` need only outlive the call: host ids are copied into the
            # library's staging, device ids are read by work of this stream
            with _as_error():
                self._plan.repair_batch(ptr, sbs, sss, optr, obs, oss, ids_ptr, sz, ns, stream=stream, flags=flags)
        return out

    def decode_batch(self, blocks, pattern_of):
        """Decoder.decode_batch_mixed with the plan's patterns (a plan made by
        Decoder.decode_plan): a new [nstripes, k, sz] tensor of every stripe's
        k primaries in order, block-major when the input was."""
        if not self._decode:
            raise Error("Precondition violation: decode_batch takes a plan made by Decoder.decode_plan")
        return self.repair_batch(blocks, pattern_of)


class Encoder(_fec.Encoder):
    """Encoder(k, m) -- see zfec/_fecmodule.c:40-44."""

    # encode(inblocks, desired_blocks_nums=None) is _fec.Encoder.encode: host
    # buffers run in C; device tensors come back to _encode_device
    # (fecmodule.cpp route_device)

    def encode_batch(self, blocks, desired_blocks_nums=None, devices=None):
        """Encode many independent stripes in one launch (fec_encode_batch).

        blocks: uint8 device tensor [nstripes, k, sz] (any strides with unit
        stride along sz; a transposed block-major [k, nstripes, sz] array is the
        fastest layout), or the same as a host numpy array, or a list of such
        device tensors (one per GPU: each runs on its own device, and a list of
        results comes back).  desired_blocks_nums: secondary block numbers in
        [k, m-1] (default k..m-1).  devices (host arrays only): a list of GPU
        indices, or "all", to split the stripes over (fec_encode_batch_multi:
        one library thread per GPU, each staging its share over its own PCIe
        link).  Returns a new [nstripes, len(desired), sz] tensor (numpy array
        for host input), block-major when the input was; device work is
        enqueued on the current stream, host calls return when done.  A batched
        counterpart of encode() for many small objects;
        no reference equivalent."""
        from . import capi

        if isinstance(blocks, (list, tuple)):
            return [self.encode_batch(b, desired_blocks_nums) for b in blocks]
        k, m = self.k, self.m
        nums = list(range(k, m)) if desired_blocks_nums is None else list(desired_blocks_nums)
        for x in nums:
            if not isinstance(x, int) or x < k or x >= m:
                raise Error("Precondition violation: encode_batch desired block nums are required to be secondary "
                            "block nums in [k, m-1] = [%d, %d], but one was %r" % (k, m - 1, x))
        ns, sz, sbs, sss, ptr = _batch_view(blocks, k, "blocks")
        devs = _devices_arg(blocks, devices)
        out = _batch_out(blocks, sss < sbs, ns, len(nums), sz)
        if nums and ns and sz:
            optr, obs, oss = _batch_strides(out)
            with _as_error():
                if devs is not None:
                    _capi_code(self).encode_batch_multi(ptr, sbs, sss, optr, obs, oss, nums, sz, ns, devs)
                else:
                    stream, flags = _batch_call_args(blocks)
                    _capi_code(self).encode_batch(ptr, sbs, sss, optr, obs, oss, nums, sz, ns, stream=stream,
                                                  flags=flags)
        return out

    def encode_ragged(self, data, sizes, offsets=None, desired_blocks_nums=None, out=None, out_offsets=None):
        """Encode many stripes of different sizes in one launch
        (fec_encode_batch_ragged).

        data and out are 1-D uint8 device tensors, the two arenas; their
        numel() are the extents no stripe may pass.  Stripe s has k blocks of
        sizes[s] bytes back to back from data[offsets[s]] (an object of k *
        sizes[s] bytes), and its r = len(desired_blocks_nums) secondary blocks
        (default k..m-1) are written back to back from out[out_offsets[s]].
        sizes, offsets and out_offsets are int64 tensors, all on data's device
        (nothing then synchronises the stream) or all on the CPU; host
        sequences of ints are taken too.  The default offsets are the packed
        layout, stripe after stripe: offsets = k * (cumsum(sizes) - sizes) and
        out_offsets = r * (cumsum(sizes) - sizes), computed on the sizes'
        device.  out=None allocates r * sizes.sum() bytes, which with sizes on
        the device costs one .item(): passing out avoids it.  A device-side
        stripe that does not fit its arena is left unwritten; a host-side one
        is an Error.  Returns (out, out_offsets)."""
        k, m = self.k, self.m
        nums = list(range(k, m)) if desired_blocks_nums is None else list(desired_blocks_nums)
        for x in nums:
            if not isinstance(x, int) or x < k or x >= m:
                raise Error("Precondition violation: encode_ragged desired block nums are required to be secondary "
                            "block nums in [k, m-1] = [%d, %d], but one was %r" % (k, m - 1, x))
        return _ragged_call(self, "encode_batch_ragged", data, sizes, offsets, out, out_offsets, nums, len(nums))

    def update_batch(self, parity, changed, new, old=None, blocknums=None):
        """Bring the stored blocks of many stripes up to date after some of
        their primaries changed, from the changed blocks alone, in place
        (fec_update_batch): the small-write path.  No other primary is read.

        parity: uint8 device tensor [nstripes, r, sz] (any strides with unit
        stride along sz): row i of a stripe holds block blocknums[i], distinct
        numbers in [0, m-1] in any order, primaries allowed (default k..m-1).
        changed: [nstripes] or [nstripes, c] integers, 1 <= c <= 4 -- a list,
        a numpy array or a torch tensor on the host or on parity's device --
        the number of the primary each input slot carries, or -1 for "none".
        new (and old): uint8 tensors [nstripes, sz] or [nstripes, c, sz] on
        parity's device, not overlapping it.  With old=None new holds the
        deltas old ^ new themselves.  The same primary in two slots is allowed:
        the two contributions add.  Host-side numbers are checked; a device-side
        number that is not in [0, k-1] makes its slot a "none".

        Afterwards every row holds what encode() gives for its block number on
        the stripe with the new primaries.  Returns parity; the work is
        enqueued on the current stream."""
        k, m = self.k, self.m
        is_tensor = type(parity).__module__.startswith("torch") and hasattr(parity, "data_ptr")
        if not is_tensor or str(parity.dtype) != "torch.uint8" or parity.dim() != 3:
            raise Error("Precondition violation: parity is required to be a uint8 device tensor [nstripes, r, sz]")
        ns, r, sz = parity.shape
        nums = _update_nums(blocknums, k, m, "update_batch")
        if len(nums) != r or r == 0:
            raise Error("Precondition violation: parity is required to hold one row per block num: %d rows, %d block "
                        "nums" % (r, len(nums)))
        if (sz > 1 and parity.stride(2) != 1) or min(parity.stride(0), parity.stride(1)) < 0:
            raise Error("Precondition violation: parity rows are required to be contiguous along sz")
        ch, ch_dev, c = _update_changed(changed, ns, k, "update_batch")
        for t, what in ((new, "new"), (old, "old")):
            if t is None and what == "old":
                continue
            ok = type(t).__module__.startswith("torch") and hasattr(t, "data_ptr") and str(t.dtype) == "torch.uint8"
            if not ok or tuple(t.shape) not in ((ns, c, sz),) + (((ns, sz),) if c == 1 else ()):
                raise Error("Precondition violation: %s is required to be a uint8 tensor [nstripes, c, sz] = "
                            "[%d, %d, %d]%s" % (what, ns, c, sz, " or [nstripes, sz]" if c == 1 else ""))
            if t.device != parity.device:
                raise Error("Precondition violation: %s is required to be on parity's device" % what)
        if not parity.is_cuda:
            raise Error("Precondition violation: parity is required to be a uint8 device tensor [nstripes, r, sz], "
                        "not a host tensor")
        if ch_dev is not None and ch_dev.device != parity.device:
            raise Error("Precondition violation: a device-side changed is required to be on parity's device")
        if ns and sz:
            import torch

            new3 = new.unsqueeze(1) if new.dim() == 2 else new
            old3 = None
            if old is not None:
                old3 = old.unsqueeze(1) if old.dim() == 2 else old
            # one pair of strides serves both inputs
            if (sz > 1 and new3.stride(2) != 1) or min(new3.stride(0), new3.stride(1)) < 0 or (
                    old3 is not None and old3.stride() != new3.stride()):
                new3 = new3.contiguous()
                old3 = old3.contiguous() if old3 is not None else None
            words, ch_ptr = _update_words(ch, ch_dev, k)
            from . import capi

            # `words` need only outlive the call: host numbers are copied into the
            # library's staging, device numbers are read by work of this stream
            with torch.cuda.device(parity.device), _as_error():
                _capi_code(self).update_batch(old3.data_ptr() if old3 is not None else 0, new3.data_ptr(),
                                              new3.stride(1), new3.stride(0), parity.data_ptr(), parity.stride(1),
                                              parity.stride(0), nums, ch_ptr, c, sz, ns,
                                              stream=_stream_handle(parity.device), flags=capi.FEC_FLAG_ASYNC)
        return parity

    def update_ragged(self, parity, sizes, changed, new, old=None, blocknums=None, offsets=None, in_offsets=None):
        """update_batch over stripes that each have their own size, in one
        launch for every code (fec_update_batch_ragged).

        parity, new (and old) are 1-D contiguous uint8 device tensors, arenas
        of packed objects: row i of stripe s is the sizes[s] bytes from
        parity[offsets[s] + i * sizes[s]] and holds block blocknums[i]
        (distinct, in [0, m-1], default k..m-1); input slot j of stripe s is
        the sizes[s] bytes from new[in_offsets[s] + j * sizes[s]], and from the
        same place in old.  With old=None new holds the deltas old ^ new.
        sizes and the offsets are lists, numpy arrays or int64 tensors, all on
        the host or all on parity's device; the default offsets are the packed
        layouts r * (cumsum(sizes) - sizes) and c * (cumsum(sizes) - sizes).
        changed is update_batch's: [nstripes] or [nstripes, c] integers, 1 <= c
        <= 4, -1 for "none", on the host or on parity's device.

        With descriptors on the device nothing synchronises with the host, and
        a stripe whose descriptor does not fit is left alone; with descriptors
        on the CPU such a stripe is an Error.  Returns parity; the work is
        enqueued on the current stream."""
        import numpy as np
        import torch

        k, m = self.k, self.m
        for t, what in ((parity, "parity"), (new, "new"), (old, "old")):
            if t is None and what == "old":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
                raise Error("Precondition violation: %s is required to be a 1-D contiguous uint8 device tensor" % what)
        nums = _update_nums(blocknums, k, m, "update_ragged")
        r = len(nums)
        if r == 0:
            raise Error("Precondition violation: update_ragged block nums are required to name at least one row")
        arrays = []
        for a, what in ((sizes, "sizes"), (offsets, "offsets"), (in_offsets, "in_offsets")):
            if a is None and what != "sizes":
                continue
            if isinstance(a, np.ndarray) and a.dtype.kind in "iu" and a.ndim == 1:
                a = a.tolist()
            arrays.append((what, _ragged_words(a, what)))
        sizes = arrays[0][1]
        ns = sizes.numel()
        for what, a in arrays[1:]:
            if a.numel() != ns:
                raise Error("Precondition violation: %s is required to hold one word per stripe: %d, not %d"
                            % (what, ns, a.numel()))
            if a.device != sizes.device:
                raise Error("Precondition violation: sizes, offsets and in_offsets are required to be all on parity's "
                            "device or all on the CPU, but sizes is on %s and %s on %s" % (sizes.device, what, a.device))
        ch, ch_dev, c = _update_changed(changed, ns, k, "update_ragged")
        if old is not None and old.numel() != new.numel():
            raise Error("Precondition violation: old is required to be an arena of new's size: %d bytes, not %d"
                        % (new.numel(), old.numel()))
        if not parity.is_cuda:
            raise Error("Precondition violation: parity is required to be a 1-D contiguous uint8 device tensor, not a "
                        "host tensor")
        for t, what in ((new, "new"), (old, "old")):
            if t is not None and t.device != parity.device:
                raise Error("Precondition violation: %s is required to be on parity's device" % what)
        if sizes.is_cuda and sizes.device != parity.device:
            raise Error("Precondition violation: sizes, offsets and in_offsets are required to be all on parity's "
                        "device or all on the CPU, but sizes is on %s and parity on %s" % (sizes.device, parity.device))
        if ch_dev is not None and ch_dev.device != parity.device:
            raise Error("Precondition violation: a device-side changed is required to be on parity's device")
        if not sizes.is_cuda:
            for what, a in arrays:
                if ns and int(a.min()) < 0:
                    raise Error("Precondition violation: %s is required to hold sizes and offsets in [0, 2^63), but "
                                "one was %d" % (what, int(a.min())))
        given = dict(arrays)
        if "offsets" not in given or "in_offsets" not in given:
            start = torch.cumsum(sizes, 0) - sizes
        offsets = given["offsets"] if "offsets" in given else r * start
        in_offsets = given["in_offsets"] if "in_offsets" in given else c * start
        if ns and parity.numel() and new.numel():
            words, ch_ptr = _update_words(ch, ch_dev, k)
            from . import capi

            # `words` and the descriptor tensors need only outlive the call: host arrays are copied
            # into the library's staging, device arrays are read by work of this stream
            with torch.cuda.device(parity.device), _as_error():
                _capi_code(self).update_batch_ragged(old.data_ptr() if old is not None else 0, new.data_ptr(),
                                                     new.numel(), 0, in_offsets.data_ptr(), parity.data_ptr(),
                                                     parity.numel(), 0, offsets.data_ptr(), sizes.data_ptr(), nums,
                                                     ch_ptr, c, ns, stream=_stream_handle(parity.device),
                                                     flags=capi.FEC_FLAG_ASYNC)
        return parity

    def _encode_device(self, inblocks, desired):
        import torch

        inblocks = list(inblocks)
        k, m = self.k, self.m
        if desired is None:
            nums = list(range(m))
        else:
            try:
                nums = list(desired)
            except TypeError:
                raise TypeError("Second argument (optional) was not a sequence.")
            for x in nums:
                if not isinstance(x, int):
                    raise Error("Precondition violation: second argument is required to contain int.")
                if x < 0 or x >= m:
                    raise Error(
                        "Precondition violation: desired block nums are required to be in [0, m-1] = [0, %d], "
                        "but one was %d" % (m - 1, x)
                    )
        bl, sz, dev = _device_blocks(inblocks, k)
        sec = [x for x in nums if x >= k]
        outs = [torch.empty(sz, dtype=torch.uint8, device=dev) for _ in sec]
        if sec and sz:
            self.encode_into(
                [b.data_ptr() for b in bl], [o.data_ptr() for o in outs], sec, sz, stream=_stream_handle(dev)
            )
        it = iter(outs)
        return [inblocks[x] if x < k else next(it) for x in nums]


class Decoder(_fec.Decoder):
    """Decoder(k, m) -- see zfec/_fecmodule.c:321-325."""

    # decode(blocks, blocknums) is _fec.Decoder.decode; device tensors come
    # back to _decode_device (fecmodule.cpp route_device)

    def decode_batch(self, blocks, blocknums, devices=None):
        """Decode many independent stripes that all received the same block
        numbers, in one launch (fec_decode_batch).

        blocks: uint8 device tensor or host numpy array [nstripes, k, sz]
        (strides as in Encoder.encode_batch), or a list of device tensors (one
        per GPU), slot j of every stripe holding block blocknums[j];
        a primary block must sit at its own slot (primary i at slot i, as
        fec_decode requires, zfec/fec.c:549).  devices: as in
        Encoder.encode_batch (fec_decode_batch_multi).  Returns a new
        [nstripes, r, sz] tensor of the r missing primaries in ascending order."""
        from . import capi

        if isinstance(blocks, (list, tuple)):
            return [self.decode_batch(b, blocknums) for b in blocks]
        k, m = self.k, self.m
        try:
            nums = list(blocknums)
        except TypeError:
            raise TypeError("Second argument was not a sequence.")
        if len(nums) != k or len(set(nums)) != k:
            raise Error("Precondition violation: blocknums is required to hold k = %d distinct block nums" % k)
        for i, x in enumerate(nums):
            if not isinstance(x, int) or x < 0 or x >= m:
                raise Error("Precondition violation: block nums are required to be in [0, m-1] = [0, %d], but one "
                            "was %r" % (m - 1, x))
            if x < k and x != i:
                raise Error("Precondition violation: decode_batch requires primary block %d at slot %d" % (x, x))
        ns, sz, sbs, sss, ptr = _batch_view(blocks, k, "blocks")
        devs = _devices_arg(blocks, devices)
        r = sum(1 for x in nums if x >= k)
        out = _batch_out(blocks, sss < sbs, ns, r, sz)
        if r and ns and sz:
            optr, obs, oss = _batch_strides(out)
            with _as_error():
                if devs is not None:
                    _capi_code(self).decode_batch_multi(ptr, sbs, sss, optr, obs, oss, nums, sz, ns, devs)
                else:
                    stream, flags = _batch_call_args(blocks)
                    _capi_code(self).decode_batch(ptr, sbs, sss, optr, obs, oss, nums, sz, ns, stream=stream,
                                                  flags=flags)
        return out

    def decode_ragged(self, data, sizes, blocknums, offsets=None, out=None, out_offsets=None):
        """Decode many stripes of different sizes that all received the same
        block numbers, in one launch (fec_decode_batch_ragged).

        Arguments as Encoder.encode_ragged: slot j of stripe s, holding block
        blocknums[j], is the sizes[s] bytes from data[offsets[s] + j *
        sizes[s]]; a primary block must sit at its own slot, as in
        decode_batch.  The r missing primaries of stripe s (ascending) are
        written back to back from out[out_offsets[s]].  Returns (out,
        out_offsets)."""
        k, m = self.k, self.m
        try:
            nums = list(blocknums)
        except TypeError:
            raise TypeError("Third argument was not a sequence.")
        if len(nums) != k or len(set(nums)) != k:
            raise Error("Precondition violation: blocknums is required to hold k = %d distinct block nums" % k)
        for i, x in enumerate(nums):
            if not isinstance(x, int) or x < 0 or x >= m:
                raise Error("Precondition violation: block nums are required to be in [0, m-1] = [0, %d], but one "
                            "was %r" % (m - 1, x))
            if x < k and x != i:
                raise Error("Precondition violation: decode_ragged requires primary block %d at slot %d" % (x, x))
        r = sum(1 for x in nums if x >= k)
        return _ragged_call(self, "decode_batch_ragged", data, sizes, offsets, out, out_offsets, nums, r)

    def decode_batch_mixed(self, blocks, blocknums):
        """Decode many independent stripes that each received their own block
        numbers, in one launch (fec_decode_batch_mixed).

        blocks: uint8 device tensor [nstripes, k, sz] (strides as in
        decode_batch).  blocknums: an [nstripes, k] integer array -- a list of
        lists, a numpy array, or a torch tensor on the host or on the device --
        row s holding the block numbers of stripe s's slots, distinct, in [0,
        m-1] and in any slot order; or a tuple (patterns [P, k], pattern_of
        [nstripes]) of the distinct rows and each stripe's index into them.
        The array form is reduced to that pair with unique() where it lives;
        a device array's ids stay on the device.  Device-side pattern_of ids
        cannot be range-checked: a stripe whose id is not below P is left
        unwritten.  Returns a new [nstripes, k, sz] tensor of every stripe's k
        primaries in order, block-major when the input was; the work is
        enqueued on the current stream.  Host (numpy) blocks are not staged by
        this call."""
        import numpy as np

        k, m = self.k, self.m
        if _is_host_array(blocks):
            raise Error("Precondition violation: decode_batch_mixed takes a device tensor; host (numpy) blocks are "
                        "not staged by this call")
        is_tensor = type(blocks).__module__.startswith("torch") and hasattr(blocks, "data_ptr")
        if not is_tensor or str(blocks.dtype) != "torch.uint8" or blocks.dim() != 3:
            raise Error("Precondition violation: blocks is required to be a uint8 device tensor [nstripes, %d, sz]" % k)
        if blocks.shape[1] != k:
            raise Error("Precondition violation: blocks is required to hold %d blocks per stripe, not %d"
                        % (k, blocks.shape[1]))
        ns = blocks.shape[0]
        ids_dev = None  # device tensor of ids, or
        ids_host = None  # numpy uint32 array of ids
        if isinstance(blocknums, tuple) and len(blocknums) == 2:
            pats, ids = blocknums
            pats = pats.cpu().numpy() if hasattr(pats, "data_ptr") else np.asarray(pats)
            if hasattr(ids, "data_ptr"):
                if ids.dim() != 1 or ids.dtype.is_floating_point:
                    raise Error("Precondition violation: pattern_of is required to be a 1-D integer array")
                nids = ids.shape[0]
                if ids.is_cuda:
                    ids_dev = ids
                else:
                    ids_host = ids.numpy()
            else:
                ids_host = np.asarray(ids)
                if ids_host.ndim != 1 or (ids_host.size and ids_host.dtype.kind not in "iu"):
                    raise Error("Precondition violation: pattern_of is required to be a 1-D integer array")
                nids = ids_host.shape[0]
            if nids != ns:
                raise Error("Precondition violation: pattern_of is required to hold nstripes = %d ids, not %d"
                            % (ns, nids))
        elif hasattr(blocknums, "data_ptr"):  # torch tensor, host or device
            import torch

            if blocknums.dim() != 2 or tuple(blocknums.shape) != (ns, k) or blocknums.dtype.is_floating_point:
                raise Error("Precondition violation: blocknums is required to be an integer array [nstripes, k] = "
                            "[%d, %d]" % (ns, k))
            upat, inv = torch.unique(blocknums, dim=0, return_inverse=True)
            pats = upat.cpu().numpy()
            if blocknums.is_cuda:
                ids_dev = inv.reshape(-1)
            else:
                ids_host = inv.reshape(-1).numpy()
        else:
            arr = np.asarray(blocknums)
            if arr.ndim != 2 or arr.shape != (ns, k) or arr.dtype.kind not in "iu":
                raise Error("Precondition violation: blocknums is required to be an integer array [nstripes, k] = "
                            "[%d, %d]" % (ns, k))
            if ns:
                pats, inv = np.unique(arr, axis=0, return_inverse=True)
            else:
                pats, inv = arr, np.zeros(0, dtype=np.int64)
            ids_host = inv.reshape(-1)
        if pats.ndim != 2 or pats.shape[1] != k or (pats.size and pats.dtype.kind not in "iu"):
            raise Error("Precondition violation: patterns is required to be an integer array [P, k = %d]" % k)
        if pats.size and (pats.min() < 0 or pats.max() >= m):
            bad = pats[(pats < 0) | (pats >= m)][0]
            raise Error("Precondition violation: block nums are required to be in [0, m-1] = [0, %d], but one was %d"
                        % (m - 1, bad))
        for row in pats:
            if len(set(row.tolist())) != k:
                raise Error("Precondition violation: the block nums of a stripe are required to be distinct, but one "
                            "stripe has %r" % (row.tolist(),))
        npat = pats.shape[0]
        if ids_host is not None and ids_host.size and (ids_host.min() < 0 or ids_host.max() >= npat):
            raise Error("Precondition violation: pattern_of ids are required to be in [0, %d]" % (npat - 1))
        if not blocks.is_cuda:
            raise Error("Precondition violation: blocks is required to be a uint8 device tensor [nstripes, %d, sz], "
                        "not a host tensor" % k)
        ns, sz, sbs, sss, ptr = _batch_view(blocks, k, "blocks")
        out = _batch_out(blocks, sss < sbs, ns, k, sz)
        if ns and sz:
            import torch

            if ids_dev is not None:
                if ids_dev.device != blocks.device:
                    raise Error("Precondition violation: device blocknums are required to be on the blocks' device")
                ids = ids_dev.to(torch.int32).contiguous()  # non-negative ids: the bits of uint32
                ids_ptr = ids.data_ptr()
            else:
                ids = np.ascontiguousarray(ids_host, dtype=np.uint32)
                ids_ptr = ids.ctypes.data
            optr, obs, oss = _batch_strides(out)
            stream, flags = _batch_call_args(blocks)
            # `ids` need only outlive the call: host ids are copied into the
            # library's staging, device ids are read by work of this stream
            with _as_error():
                _capi_code(self).decode_batch_mixed(ptr, sbs, sss, optr, obs, oss,
                                                    np.ascontiguousarray(pats, dtype=np.uint32), ids_ptr, sz, ns,
                                                    stream=stream, flags=flags)
        return out

    def repair_batch(self, blocks, blocknums, targets, out=None):
        """Rebuild any lost blocks, primaries and parity alike, of many
        independent stripes that each hold their own k blocks, in one launch
        (fec_repair_batch).

        blocks: uint8 device tensor [nstripes, k, sz] (strides as in
        decode_batch_mixed).  blocknums: an [nstripes, k] integer array -- a
        list of lists, a numpy array, or a torch tensor on the host or on the
        device -- row s holding the block numbers of stripe s's slots,
        distinct, in [0, m-1] and in any slot order.  targets: an [nstripes, t]
        integer array of the same kinds, 1 <= t <= 32: row s lists the block
        numbers to rebuild for stripe s, in [0, m-1], or -1 for "none" (a stripe
        that lost fewer than t blocks).  A target that is also present is
        copied; duplicates are allowed.  Alternatively blocknums is a tuple
        (patterns [P, k], pattern_of [nstripes]) and targets is [P, t], one row
        per pattern.  The array form is reduced to that with unique() over the
        concatenated [nstripes, k + t] rows where the arrays live; a device
        array's ids stay on the device.  Device-side pattern_of ids cannot be
        range-checked: a stripe whose id is not below P is left unwritten.

        Returns [nstripes, t, sz]: row i of stripe s is block targets[s][i] of
        that stripe, bit-identical to decode followed by encode.  With out=None
        a new tensor is allocated (block-major when the input was) and the rows
        of -1 targets are unspecified; with out (a uint8 tensor of that shape
        on the blocks' device, contiguous along sz, not overlapping blocks) the
        rows of -1 targets keep their contents, and out is returned.  The work
        is enqueued on the current stream.  Host (numpy) blocks are not staged
        by this call."""
        import numpy as np

        k, m = self.k, self.m
        if _is_host_array(blocks):
            raise Error("Precondition violation: repair_batch takes a device tensor; host (numpy) blocks are not "
                        "staged by this call")
        is_tensor = type(blocks).__module__.startswith("torch") and hasattr(blocks, "data_ptr")
        if not is_tensor or str(blocks.dtype) != "torch.uint8" or blocks.dim() != 3:
            raise Error("Precondition violation: blocks is required to be a uint8 device tensor [nstripes, %d, sz]" % k)
        if blocks.shape[1] != k:
            raise Error("Precondition violation: blocks is required to hold %d blocks per stripe, not %d"
                        % (k, blocks.shape[1]))
        ns = blocks.shape[0]

        pats, tgts, ids_host, ids_dev = self._repair_patterns(ns, blocknums, targets)
        t, npat = tgts.shape[1], pats.shape[0]
        sz = blocks.shape[2]
        if out is not None:
            out_ok = type(out).__module__.startswith("torch") and hasattr(out, "data_ptr")
            if not out_ok or str(out.dtype) != "torch.uint8" or tuple(out.shape) != (ns, t, sz):
                raise Error("Precondition violation: out is required to be a uint8 tensor [nstripes, t, sz] = "
                            "[%d, %d, %d]" % (ns, t, sz))
            if out.device != blocks.device:
                raise Error("Precondition violation: out is required to be on the blocks' device")
            if (sz > 1 and out.stride(2) != 1) or min(out.stride(0), out.stride(1)) < 0:
                raise Error("Precondition violation: out rows are required to be contiguous along sz")
        if not blocks.is_cuda:
            raise Error("Precondition violation: blocks is required to be a uint8 device tensor [nstripes, %d, sz], "
                        "not a host tensor" % k)
        ns, sz, sbs, sss, ptr = _batch_view(blocks, k, "blocks")
        if out is None:
            out = _batch_out(blocks, sss < sbs, ns, t, sz)
        if ns and sz and npat:
            import torch

            if ids_dev is not None:
                if ids_dev.device != blocks.device:
                    raise Error("Precondition violation: device blocknums are required to be on the blocks' device")
                ids = ids_dev.to(torch.int32).contiguous()  # non-negative ids: the bits of uint32
                ids_ptr = ids.data_ptr()
            else:
                ids = np.ascontiguousarray(ids_host, dtype=np.uint32)
                ids_ptr = ids.ctypes.data
            optr, obs, oss = _batch_strides(out)
            stream, flags = _batch_call_args(blocks)
            # `ids` need only outlive the call: host ids are copied into the
            # library's staging, device ids are read by work of this stream
            with _as_error():
                _capi_code(self).repair_batch(ptr, sbs, sss, optr, obs, oss, np.ascontiguousarray(pats, dtype=np.int64),
                                              np.ascontiguousarray(tgts, dtype=np.int64), ids_ptr, sz, ns,
                                              stream=stream, flags=flags)
        return out

    def _repair_patterns(self, ns, blocknums, targets):
        """The two forms of repair_batch's blocknums and targets reduced to
        patterns: (patterns [P, k], targets [P, t], ids_host, ids_dev), numpy
        tables checked against k and m, and the nstripes pattern ids as a
        numpy array or a device tensor (the other None)."""
        import numpy as np

        k, m = self.k, self.m

        def host_table(x, what):
            a = x.cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
            if a.ndim != 2 or (a.size and a.dtype.kind not in "iu"):
                raise Error("Precondition violation: %s is required to be a 2-D integer array" % what)
            return a

        ids_dev = None  # device tensor of ids, or
        ids_host = None  # numpy array of ids
        if isinstance(blocknums, tuple) and len(blocknums) == 2:
            pats, ids = blocknums
            pats = host_table(pats, "patterns")
            tgts = host_table(targets, "targets")
            if tgts.shape[0] != pats.shape[0]:
                raise Error("Precondition violation: targets is required to hold one row per pattern: %d rows, %d "
                            "patterns" % (tgts.shape[0], pats.shape[0]))
            if hasattr(ids, "data_ptr"):
                if ids.dim() != 1 or ids.dtype.is_floating_point:
                    raise Error("Precondition violation: pattern_of is required to be a 1-D integer array")
                nids = ids.shape[0]
                if ids.is_cuda:
                    ids_dev = ids
                else:
                    ids_host = ids.numpy()
            else:
                ids_host = np.asarray(ids)
                if ids_host.ndim != 1 or (ids_host.size and ids_host.dtype.kind not in "iu"):
                    raise Error("Precondition violation: pattern_of is required to be a 1-D integer array")
                nids = ids_host.shape[0]
            if nids != ns:
                raise Error("Precondition violation: pattern_of is required to hold nstripes = %d ids, not %d"
                            % (ns, nids))
        else:
            def stripe_table(x, what, width):
                if hasattr(x, "data_ptr"):  # torch tensor, host or device
                    a, ok = x, x.dim() == 2 and not x.dtype.is_floating_point
                else:
                    a = np.asarray(x)
                    ok = a.ndim == 2 and (a.dtype.kind in "iu" or not a.size)
                if not ok or a.shape[0] != ns or (width is not None and a.shape[1] != width):
                    raise Error("Precondition violation: %s is required to be an integer array [nstripes, %s] = "
                                "[%d, %s]" % (what, "t" if width is None else "k", ns, "t" if width is None else width))
                return a

            tabs = [stripe_table(blocknums, "blocknums", k), stripe_table(targets, "targets", None)]
            on_dev = [x for x in tabs if hasattr(x, "data_ptr") and x.is_cuda]
            if on_dev:
                import torch

                both = torch.cat([torch.as_tensor(x).to(on_dev[0].device).long() for x in tabs], dim=1)
                urows, inv = torch.unique(both, dim=0, return_inverse=True)
                urows = urows.cpu().numpy()
                ids_dev = inv.reshape(-1)
            else:
                both = np.concatenate([x.numpy() if hasattr(x, "data_ptr") else x for x in tabs],
                                      axis=1).astype(np.int64)
                if ns:
                    urows, inv = np.unique(both, axis=0, return_inverse=True)
                else:
                    urows, inv = both, np.zeros(0, dtype=np.int64)
                ids_host = inv.reshape(-1)
            pats, tgts = urows[:, :k], urows[:, k:]
        if pats.shape[1] != k:
            raise Error("Precondition violation: patterns is required to be an integer array [P, k = %d]" % k)
        t = tgts.shape[1]
        if t < 1 or t > 32:
            raise Error("Precondition violation: targets is required to hold between 1 and 32 block nums per stripe, "
                        "not %d" % t)
        if pats.size and (pats.min() < 0 or pats.max() >= m):
            bad = pats[(pats < 0) | (pats >= m)][0]
            raise Error("Precondition violation: block nums are required to be in [0, m-1] = [0, %d], but one was %d"
                        % (m - 1, bad))
        for row in pats:
            if len(set(row.tolist())) != k:
                raise Error("Precondition violation: the block nums of a stripe are required to be distinct, but one "
                            "stripe has %r" % (row.tolist(),))
        if tgts.size and (tgts.min() < -1 or tgts.max() >= m):
            bad = tgts[(tgts < -1) | (tgts >= m)][0]
            raise Error("Precondition violation: targets are required to be in [0, m-1] = [0, %d] or -1 (none), but "
                        "one was %d" % (m - 1, bad))
        npat = pats.shape[0]
        if ids_host is not None and ids_host.size and (ids_host.min() < 0 or ids_host.max() >= npat):
            raise Error("Precondition violation: pattern_of ids are required to be in [0, %d]" % (npat - 1))
        return pats, tgts, ids_host, ids_dev

    def repair_ragged(self, data, sizes, blocknums, targets, offsets=None, out=None, out_offsets=None):
        """repair_batch over stripes that each have their own size, in one
        launch (fec_repair_batch_ragged).

        data, sizes, offsets, out and out_offsets as in decode_ragged: slot j
        of stripe s is the sizes[s] bytes from data[offsets[s] + j *
        sizes[s]], and row i of stripe s is written from out[out_offsets[s] +
        i * sizes[s]]; the defaults are the packed layouts k * (cumsum(sizes)
        - sizes) and t * (cumsum(sizes) - sizes).  blocknums and targets take
        the two forms repair_batch accepts: [nstripes, k] with [nstripes, t],
        or (patterns [P, k], pattern_of [nstripes]) with [P, t]; a target of
        -1 means none.  Returns the output arena; with out given, the rows of
        -1 targets keep their contents, without it they are unspecified.  With
        descriptors on the device nothing synchronises with the host, and a
        stripe whose descriptor does not fit, or whose device-side id is not
        below P, is left unwritten; with descriptors on the CPU such a stripe
        is an Error.  A decode with a pattern per stripe is targets =
        0..k-1."""
        import numpy as np
        import torch

        sizes = _ragged_words(sizes, "sizes")
        ns = sizes.numel()
        pats, tgts, ids_host, ids_dev = self._repair_patterns(ns, blocknums, targets)
        t = tgts.shape[1]
        if ids_dev is not None:
            if not isinstance(data, torch.Tensor) or ids_dev.device != data.device:
                raise Error("Precondition violation: device blocknums are required to be on the data's device")
            ids = ids_dev.to(torch.int32).contiguous()  # non-negative ids: the bits of uint32
            ids_ptr = ids.data_ptr()
        else:
            ids = np.ascontiguousarray(ids_host, dtype=np.uint32)
            ids_ptr = ids.ctypes.data
        pats = np.ascontiguousarray(pats, dtype=np.int64)
        tgts = np.ascontiguousarray(tgts, dtype=np.int64)

        code = _capi_code(self)

        def call(src, src_bytes, sbs, soff, dst, dst_bytes, dbs, doff, szs, nums, nstripes, stream=0):
            # `ids` need only outlive the call: host ids are copied into the
            # library's staging, device ids are read by work of this stream
            code.repair_batch_ragged(src, src_bytes, sbs, soff, dst, dst_bytes, dbs, doff, szs, pats, tgts, ids_ptr,
                                     nstripes, stream=stream)

        return _ragged_call(self, call, data, sizes, offsets, out, out_offsets, None, t)[0]

    def repair_plan(self, patterns, targets):
        """A RepairPlan of P erasure patterns for repair_batch's work: patterns
        is an integer array [P, k] (list of lists, numpy array or torch tensor)
        of the block numbers a stripe's slots hold, distinct, in [0, m-1], in
        any slot order; targets an integer array [P, t], 1 <= t <= 32, of the
        block numbers to rebuild, in [0, m-1] or -1 for none.  The plan lives
        on the current device."""
        return self._plan(patterns, targets, False)

    def decode_plan(self, patterns):
        """A RepairPlan whose every pattern rebuilds primaries 0..k-1 in order:
        decode_batch_mixed's work (k <= 32)."""
        import numpy as np

        if self.k > 32:
            raise Error("Precondition violation: decode_plan takes codes of k <= 32, not k = %d (a plan holds at most "
                        "32 rows per pattern)" % self.k)
        pats = patterns.cpu().numpy() if hasattr(patterns, "data_ptr") else np.asarray(patterns)
        n = pats.shape[0] if pats.ndim == 2 else 0
        return self._plan(pats, np.tile(np.arange(self.k, dtype=np.int64), (n, 1)), True)

    def _plan(self, patterns, targets, decode):
        import numpy as np

        k, m = self.k, self.m

        def host_table(x, what):
            a = x.cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
            if a.ndim != 2 or (a.size and a.dtype.kind not in "iu"):
                raise Error("Precondition violation: %s is required to be a 2-D integer array" % what)
            return a

        pats, tgts = host_table(patterns, "patterns"), host_table(targets, "targets")
        if pats.shape[1] != k:
            raise Error("Precondition violation: patterns is required to be an integer array [P, k = %d]" % k)
        if pats.shape[0] < 1:
            raise Error("Precondition violation: patterns is required to hold at least one pattern")
        if tgts.shape[0] != pats.shape[0]:
            raise Error("Precondition violation: targets is required to hold one row per pattern: %d rows, %d "
                        "patterns" % (tgts.shape[0], pats.shape[0]))
        t = tgts.shape[1]
        if t < 1 or t > 32:
            raise Error("Precondition violation: targets is required to hold between 1 and 32 block nums per pattern, "
                        "not %d" % t)
        if pats.min() < 0 or pats.max() >= m:
            bad = pats[(pats < 0) | (pats >= m)][0]
            raise Error("Precondition violation: block nums are required to be in [0, m-1] = [0, %d], but one was %d"
                        % (m - 1, bad))
        for row in pats:
            if len(set(row.tolist())) != k:
                raise Error("Precondition violation: the block nums of a stripe are required to be distinct, but one "
                            "stripe has %r" % (row.tolist(),))
        if tgts.min() < -1 or tgts.max() >= m:
            bad = tgts[(tgts < -1) | (tgts >= m)][0]
            raise Error("Precondition violation: targets are required to be in [0, m-1] = [0, %d] or -1 (none), but "
                        "one was %d" % (m - 1, bad))
        return RepairPlan(self, pats.astype(np.int64), tgts.astype(np.int64), decode)

    def verify_batch(self, blocks, blocknums):
        """Check many independent stripes for consistency without writing any
        block (scrubbing; fec_verify_batch).

        blocks: uint8 device tensor [nstripes, nb, sz] (strides as in
        decode_batch), slot j of every stripe holding block blocknums[j].
        blocknums: nb distinct ints in [0, m-1], in any order, with
        k + 1 <= nb <= m; the first k slots are the basis, the other nb - k the
        checks.  Returns a torch.bool tensor [nstripes, nb - k] on the blocks'
        device: True where a check block differs, in at least one byte, from
        what the basis blocks imply.  A corrupt check block sets only its own
        column; one corrupt basis block sets every column of its stripe.  The
        work is enqueued on the current stream, without a host sync.  Host
        (numpy) blocks are not staged by this call."""
        import torch

        nums, nb, ns, sz, sbs, sss, ptr = self._scrub_args(blocks, blocknums, "verify_batch")
        c = nb - self.k
        words = (c + 31) // 32
        if not (ns and sz):
            return torch.zeros((ns, c), dtype=torch.bool, device=blocks.device)
        mask = torch.empty((ns, words), dtype=torch.int32, device=blocks.device)  # the library clears it
        stream, flags = _batch_call_args(blocks)
        with _as_error():
            _capi_code(self).verify_batch(ptr, sbs, sss, nums, sz, ns, mask.data_ptr(), stream=stream, flags=flags)
        shifts = torch.arange(32, dtype=torch.int32, device=blocks.device)
        bits = (mask.unsqueeze(-1) >> shifts) & 1
        return bits.reshape(ns, words * 32)[:, :c].ne(0)

    def locate_batch(self, blocks, blocknums):
        """Name the corrupt block of every stripe (fec_locate_batch): the step
        between verify_batch and repair_batch.

        blocks and blocknums as in verify_batch, with the same preconditions.
        Returns a torch.int32 tensor [nstripes] on the blocks' device: a value
        >= 0 is the SLOT (an index into blocknums, not a block number) of the
        stripe's one corrupt block; LOCATE_CLEAN (-1) says the stripe is
        consistent, LOCATE_MANY (-2) that more than one block is corrupt,
        LOCATE_UNKNOWN (-3) that a single check (nb == k + 1) cannot tell
        which block it is.  With two or more checks a stripe with exactly one
        corrupt block always gets that block's slot.  The work is enqueued on
        the current stream, without a host sync."""
        import torch

        nums, nb, ns, sz, sbs, sss, ptr = self._scrub_args(blocks, blocknums, "locate_batch")
        if not (ns and sz):
            return torch.full((ns,), LOCATE_CLEAN, dtype=torch.int32, device=blocks.device)
        out = torch.empty((ns,), dtype=torch.int32, device=blocks.device)
        stream, flags = _batch_call_args(blocks)
        with _as_error():
            _capi_code(self).locate_batch(ptr, sbs, sss, nums, sz, ns, out.data_ptr(), stream=stream, flags=flags)
        return out

    def verify_ragged(self, data, sizes, blocknums, offsets=None):
        """verify_batch over stripes that each have their own size, in one
        launch (fec_verify_batch_ragged).

        data: 1-D contiguous uint8 device tensor, the arena; data.numel() is
        its extent.  sizes: one block size per stripe, a 1-D int64 tensor (on
        the data's device or the CPU) or a sequence of ints.  Stripe s is the
        packed object of nb = len(blocknums) blocks of sizes[s] bytes from
        data[offsets[s]], slot j holding block blocknums[j] (blocknums as in
        verify_batch).  offsets defaults to nb * (cumsum(sizes) - sizes),
        computed on the sizes' device.  Returns a torch.bool tensor
        [nstripes, nb - k] on the data's device, as verify_batch does; a
        zero-size stripe has no bit set.  With descriptors on the device
        nothing synchronises with the host, and a stripe whose descriptor does
        not fit the data is not read and has EVERY bit set; with descriptors
        on the CPU such a stripe is an Error."""
        import torch

        nums, ns, szs, offs = self._ragged_scrub_args(data, sizes, blocknums, offsets)
        c = len(nums) - self.k
        words = (c + 31) // 32
        if not ns:
            return torch.zeros((0, c), dtype=torch.bool, device=data.device)
        mask = torch.empty((ns, words), dtype=torch.int32, device=data.device)  # the library clears it
        with torch.cuda.device(data.device), _as_error():
            _capi_code(self).verify_batch_ragged(data.data_ptr(), data.numel(), 0, offs.data_ptr(), szs.data_ptr(),
                                                 nums, ns, mask.data_ptr(), stream=_stream_handle(data.device))
        shifts = torch.arange(32, dtype=torch.int32, device=data.device)
        bits = (mask.unsqueeze(-1) >> shifts) & 1
        return bits.reshape(ns, words * 32)[:, :c].ne(0)

    def locate_ragged(self, data, sizes, blocknums, offsets=None):
        """locate_batch over stripes that each have their own size, in one
        launch (fec_locate_batch_ragged).

        Arguments as verify_ragged.  Returns a torch.int32 tensor [nstripes]
        on the data's device with locate_batch's verdicts; a zero-size stripe
        is LOCATE_CLEAN, and with descriptors on the device a stripe whose
        descriptor does not fit the data is not read and is LOCATE_UNFIT
        (-5)."""
        import torch

        nums, ns, szs, offs = self._ragged_scrub_args(data, sizes, blocknums, offsets)
        out = torch.empty((ns,), dtype=torch.int32, device=data.device)
        if ns:
            with torch.cuda.device(data.device), _as_error():
                _capi_code(self).locate_batch_ragged(data.data_ptr(), data.numel(), 0, offs.data_ptr(), szs.data_ptr(),
                                                     nums, ns, out.data_ptr(), stream=_stream_handle(data.device))
        return out

    def correct_ragged(self, data, sizes, blocknums, offsets=None):
        """correct_batch over stripes that each have their own size: scrub,
        locate and heal in place, in one call (fec_correct_batch_ragged).

        Arguments as locate_ragged.  Returns the torch.int32 verdict tensor
        [nstripes] locate_ragged would return for the data as it was on entry
        (LOCATE_UNFIT included), and CORRECTS `data` IN PLACE: in a stripe
        whose verdict is a slot h >= 0, the sizes[s] bytes of slot h are
        rewritten from k other slots of that stripe, as correct_batch does.
        Nothing else is written: no byte of a clean, LOCATE_MANY,
        LOCATE_UNKNOWN, LOCATE_UNFIT or zero-size stripe, no other slot of a
        corrected stripe, no byte past sizes[s] of slot h.  The work is
        enqueued on the current stream."""
        import torch

        nums, ns, szs, offs = self._ragged_scrub_args(data, sizes, blocknums, offsets)
        out = torch.empty((ns,), dtype=torch.int32, device=data.device)
        if ns:
            with torch.cuda.device(data.device), _as_error():
                _capi_code(self).correct_batch_ragged(data.data_ptr(), data.numel(), 0, offs.data_ptr(),
                                                      szs.data_ptr(), nums, ns, out.data_ptr(),
                                                      stream=_stream_handle(data.device))
        return out

    def locate2_ragged(self, data, sizes, blocknums, offsets=None):
        """locate2_batch over stripes that each have their own size, in one
        call (fec_locate2_batch_ragged).

        Arguments as locate_ragged.  Returns a torch.int32 tensor
        [2, nstripes] on the data's device.  Column s is what locate2_batch
        gives for stripe s alone: (a, b), a < b, the SLOTS of its two corrupt
        blocks, or (v, LOCATE_NONE) with v what locate_ragged returns,
        LOCATE_CLEAN for a zero-size stripe and LOCATE_UNFIT (-5) included.
        Pairs are looked for with nb - k >= 4 checks and nb <= 32 blocks per
        stripe; other shapes get locate_ragged's verdicts."""
        return self._scrub2_ragged(data, sizes, blocknums, offsets, "locate2_batch_ragged")

    def correct2_ragged(self, data, sizes, blocknums, offsets=None):
        """correct2_batch over stripes that each have their own size: scrub,
        locate and heal up to two blocks per stripe in place, in one call
        (fec_correct2_batch_ragged).

        Arguments as locate_ragged.  Returns the torch.int32 verdicts
        [2, nstripes] locate2_ragged would return for the data as it was on
        entry, and CORRECTS `data` IN PLACE: a single slot exactly as
        correct_ragged does, and for a pair (a, b) the sizes[s] bytes of slots
        a and b, from the k lowest other slots of the stripe.  Nothing else is
        written: no byte of a clean, LOCATE_MANY, LOCATE_UNKNOWN, LOCATE_UNFIT
        or zero-size stripe, no other slot of a healed stripe, no byte past
        sizes[s] of a rewritten slot.  The work is enqueued on the current
        stream."""
        return self._scrub2_ragged(data, sizes, blocknums, offsets, "correct2_batch_ragged")

    def _scrub2_ragged(self, data, sizes, blocknums, offsets, what):
        import torch

        nums, ns, szs, offs = self._ragged_scrub_args(data, sizes, blocknums, offsets)
        out = torch.empty((2, ns), dtype=torch.int32, device=data.device)
        if ns:
            with torch.cuda.device(data.device), _as_error():
                getattr(_capi_code(self), what)(data.data_ptr(), data.numel(), 0, offs.data_ptr(), szs.data_ptr(),
                                                nums, ns, out.data_ptr(), stream=_stream_handle(data.device))
        return out

    def _ragged_scrub_args(self, data, sizes, blocknums, offsets):
        """The preconditions of verify_ragged / locate_ragged; returns
        (nums, nstripes, sizes, offsets), the two descriptor tensors on one device."""
        import torch

        nums = self._scrub_nums(blocknums)
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1 \
                or not data.is_contiguous():
            raise Error("Precondition violation: data is required to be a 1-D contiguous uint8 device tensor")
        sizes = _ragged_words(sizes, "sizes")
        ns = sizes.numel()
        if offsets is not None:
            offsets = _ragged_words(offsets, "offsets")
            if offsets.numel() != ns:
                raise Error("Precondition violation: offsets is required to hold one word per stripe: %d, not %d"
                            % (ns, offsets.numel()))
            if offsets.device != sizes.device:
                raise Error("Precondition violation: sizes and offsets are required to be both on the data's device "
                            "or both on the CPU, but sizes is on %s and offsets on %s"
                            % (sizes.device, offsets.device))
        if sizes.is_cuda and sizes.device != data.device:
            raise Error("Precondition violation: sizes and offsets are required to be both on the data's device or "
                        "both on the CPU, but sizes is on %s and data on %s" % (sizes.device, data.device))
        if not sizes.is_cuda:
            for what, a in (("sizes", sizes), ("offsets", offsets)):
                if a is not None and ns and int(a.min()) < 0:
                    raise Error("Precondition violation: %s is required to hold sizes and offsets in [0, 2^63), but "
                                "one was %d" % (what, int(a.min())))
        if not _is_device_tensor(data):
            raise Error("Precondition violation: data is required to be a uint8 tensor on a GPU")
        if offsets is None:  # the packed object-major layout: stripe after stripe, a stripe's blocks back to back
            offsets = len(nums) * (torch.cumsum(sizes, 0) - sizes)
        return nums, ns, sizes, offsets

    def correct_batch(self, blocks, blocknums):
        """Scrub, locate and heal in place, in one call (fec_correct_batch).

        blocks and blocknums as in locate_batch, with the same preconditions.
        Returns the torch.int32 verdict tensor [nstripes] locate_batch would
        return for the blocks as they were on entry, and CORRECTS `blocks` IN
        PLACE: in a stripe whose verdict is a slot h >= 0, the sz bytes of slot
        h are rewritten from k other slots of that stripe (slots 0..k-1, check
        0 standing in for h when h < k).  Nothing else is written: no byte of a
        LOCATE_CLEAN, LOCATE_MANY or LOCATE_UNKNOWN stripe, no other slot of a
        corrected stripe, nothing past a row's sz bytes.  Every corrected
        stripe is consistent afterwards (verify_batch returns no bit for it).
        With two or more checks a stripe with exactly one corrupt block is
        restored bit for bit.  With exactly two checks, two blocks corrupt at
        one byte position can be taken for a third and miscorrected: pass
        nb >= k + 3 to have every double error refused (LOCATE_MANY) instead.
        With one check nothing is ever rewritten.  The work is enqueued on the
        current stream, without a host sync."""
        import torch

        nums, nb, ns, sz, sbs, sss, ptr = self._scrub_args(blocks, blocknums, "correct_batch")
        if not (ns and sz):
            return torch.full((ns,), LOCATE_CLEAN, dtype=torch.int32, device=blocks.device)
        out = torch.empty((ns,), dtype=torch.int32, device=blocks.device)
        stream, flags = _batch_call_args(blocks)
        with _as_error():
            _capi_code(self).correct_batch(ptr, sbs, sss, nums, sz, ns, out.data_ptr(), stream=stream, flags=flags)
        return out

    def locate2_batch(self, blocks, blocknums):
        """Name up to two corrupt blocks of every stripe (fec_locate2_batch).

        blocks and blocknums as in locate_batch, with the same preconditions.
        Returns a torch.int32 tensor [2, nstripes] on the blocks' device.
        Column s is (a, b), a < b, the SLOTS of the stripe's two corrupt
        blocks, or (v, LOCATE_NONE) with v what locate_batch returns: a single
        slot, LOCATE_CLEAN, LOCATE_UNKNOWN or LOCATE_MANY.  Pairs are looked
        for with nb - k >= 4 checks and nb <= 32 blocks per stripe; other
        shapes get locate_batch's verdicts.  With four or more checks a stripe
        with exactly two corrupt blocks always gets that pair; pass nb >= k + 5
        to have triple errors refused (LOCATE_MANY).  The work is enqueued on
        the current stream, without a host sync."""
        return self._scrub2(blocks, blocknums, "locate2_batch")

    def correct2_batch(self, blocks, blocknums):
        """Scrub, locate and heal up to two blocks per stripe in place, in one
        call (fec_correct2_batch).

        Returns the torch.int32 verdicts [2, nstripes] locate2_batch would
        return for the blocks as they were on entry, and CORRECTS `blocks` IN
        PLACE: a single slot exactly as correct_batch does, and for a pair
        (a, b) the sz bytes of slots a and b, from the k lowest other slots of
        the stripe.  Nothing else is written.  Every corrected stripe is
        consistent afterwards (verify_batch returns no bit for it)."""
        return self._scrub2(blocks, blocknums, "correct2_batch")

    def _scrub2(self, blocks, blocknums, what):
        import torch

        nums, nb, ns, sz, sbs, sss, ptr = self._scrub_args(blocks, blocknums, what)
        out = torch.empty((2, ns), dtype=torch.int32, device=blocks.device)
        if not (ns and sz):
            out[0] = LOCATE_CLEAN
            out[1] = LOCATE_NONE
            return out
        stream, flags = _batch_call_args(blocks)
        with _as_error():
            getattr(_capi_code(self), what)(ptr, sbs, sss, nums, sz, ns, out.data_ptr(), stream=stream, flags=flags)
        return out

    def _scrub_args(self, blocks, blocknums, what):
        """The preconditions the scrub calls (verify_batch to correct2_batch) share; returns
        (nums, nb, nstripes, sz, block stride, stripe stride, address)."""
        import torch

        if _is_host_array(blocks):
            raise Error("Precondition violation: %s takes a device tensor; host (numpy) blocks are not "
                        "staged by this call" % what)
        nums = self._scrub_nums(blocknums)
        nb = len(nums)
        is_tensor = type(blocks).__module__.startswith("torch") and hasattr(blocks, "data_ptr")
        if not is_tensor or blocks.dtype != torch.uint8 or blocks.dim() != 3:
            raise Error("Precondition violation: blocks is required to be a uint8 device tensor [nstripes, %d, sz]"
                        % nb)
        if blocks.shape[1] != nb:
            raise Error("Precondition violation: blocks is required to hold %d blocks per stripe, not %d"
                        % (nb, blocks.shape[1]))
        if not blocks.is_cuda:
            raise Error("Precondition violation: blocks is required to be a uint8 device tensor [nstripes, %d, sz], "
                        "not a host tensor" % nb)
        ns, sz, sbs, sss, ptr = _batch_view(blocks, nb, "blocks")
        return nums, nb, ns, sz, sbs, sss, ptr

    def _scrub_nums(self, blocknums):
        """The block numbers of a scrub call as a list: k + 1 to m distinct ints in [0, m-1]."""
        k, m = self.k, self.m
        try:
            nums = list(blocknums)
        except TypeError:
            raise TypeError("Second argument was not a sequence.")
        nb = len(nums)
        if nb <= k or nb > m:
            raise Error("Precondition violation: blocknums is required to hold between k + 1 = %d and m = %d block "
                        "nums, not %d" % (k + 1, m, nb))
        for x in nums:
            if not isinstance(x, int) or x < 0 or x >= m:
                raise Error("Precondition violation: block nums are required to be in [0, m-1] = [0, %d], but one "
                            "was %r" % (m - 1, x))
        if len(set(nums)) != nb:
            raise Error("Precondition violation: block nums are required to be distinct, but got %r" % (nums,))
        return nums

    def _check_blocknums(self, blocknums):
        """Validated list of k block numbers (the reference's checks,
        zfec/_fecmodule.c:429-472, plus distinctness)."""
        k, m = self.k, self.m
        try:
            nums = list(blocknums)
        except TypeError:
            raise TypeError("Second argument was not a sequence.")
        if len(nums) != k:
            raise Error(
                "Precondition violation: Wrong length -- blocknums is required to contain exactly k blocks.  "
                "len(blocknums): %d, k: %d" % (len(nums), k)
            )
        for x in nums:
            if not isinstance(x, int):
                raise Error("Precondition violation: second argument is required to contain int.")
            if x < 0 or x > 255:
                raise Error("Precondition violation: block nums can't be less than zero or greater than 255.  %d\n" % x)
            if x >= m:
                raise Error(
                    "Precondition violation: block nums are required to be less than m = %d, but one was %d" % (m, x)
                )
        if len(set(nums)) != k:
            raise Error("Precondition violation: block nums are required to be distinct")
        return nums

    def _decode_device(self, blocks, blocknums):
        blocks = list(blocks)
        import torch

        k = self.k
        nums = self._check_blocknums(blocknums)
        bl, sz, dev = _device_blocks(blocks, k)
        objs = list(blocks)
        # primary i into slot i (zfec/_fecmodule.c:482-493)
        i = 0
        while i < k:
            c = nums[i]
            if c >= k or c == i:
                i += 1
            else:
                nums[i], nums[c] = nums[c], nums[i]
                bl[i], bl[c] = bl[c], bl[i]
                objs[i], objs[c] = objs[c], objs[i]
        missing = [i for i in range(k) if nums[i] >= k]
        outs = [torch.empty(sz, dtype=torch.uint8, device=dev) for _ in missing]
        if missing and sz:
            self.decode_into(
                [b.data_ptr() for b in bl], [o.data_ptr() for o in outs], nums, sz, stream=_stream_handle(dev)
            )
        it = iter(outs)
        return [objs[i] if nums[i] == i else next(it) for i in range(k)]


from . import easyfec  # noqa: E402  (needs Encoder/Decoder above)
from . import filefec, cmdline_zfec, cmdline_zunfec  # noqa: E402  (as zfec/__init__.py imports them)


def reuse_host_memory(keep_bytes=1 << 30, mmap_threshold=32 << 20):
    """Let this process's C allocator (glibc) keep freed blocks for reuse.

    Output ``bytes`` of large host-memory calls are new objects; by default glibc
    serves each one of more than a few MiB with fresh pages (mmap, or a heap it
    trims on free), so every call faults them in and every free returns them to
    the kernel.  On the MI355X host that is most of a K=3/M=10 64 MiB encode from
    ``bytes``: 3.0 GB/s per call with the freeing counted, 15.5 GB/s when blocks
    are reused (tools/e2e_host.py).  This sets
    M_MMAP_THRESHOLD (blocks under ``mmap_threshold`` come from the heap; glibc
    caps it at 32 MiB) and M_TRIM_THRESHOLD (up to ``keep_bytes`` of free heap is
    kept), the same as ``GLIBC_TUNABLES=glibc.malloc.mmap_threshold=...:
    glibc.malloc.trim_threshold=...`` at start-up.  It is process-wide, so it is
    opt-in.  Returns True if glibc accepted both settings.
    """
    import ctypes
    import ctypes.util

    try:
        libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
        mallopt = libc.mallopt
    except (OSError, AttributeError):
        return False
    mallopt.argtypes = [ctypes.c_int, ctypes.c_int]
    mallopt.restype = ctypes.c_int
    M_TRIM_THRESHOLD, M_MMAP_THRESHOLD = -1, -3
    ok = mallopt(M_MMAP_THRESHOLD, int(min(mmap_threshold, 32 << 20))) == 1
    return mallopt(M_TRIM_THRESHOLD, int(min(keep_bytes, (1 << 31) - 1))) == 1 and ok
