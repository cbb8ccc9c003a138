"""What every device-buffer call shares: torch as plumbing, the call's stream, a read-back on that
stream, the CRC output tensor and the "empty means NULL" rule for pointers."""
from __future__ import annotations

from . import _lib


def _torch():
    if _lib.torch is None:
        raise RuntimeError("device-buffer calls need torch (ROCm) for device memory")
    return _lib.torch


# The stream contract of every device-buffer call of the package.  ``stream=None`` is torch's current
# stream.  ``stream=s`` alone is enough: every launch, memset and copy of the call -- the
# library's and the wrapper's own, a read-back included -- goes to ``s`` and to no other stream,
# whatever torch's current stream is and however busy it is; the wrapper allocates (``t.empty``,
# no fill) and does nothing else on the device.  What the caller owes: the inputs are ready in
# ``s``'s order, and the tensors handed in and returned stay alive until ``s`` has run the call
# (torch's allocator knows the current stream only).  ``s`` is a ``torch.cuda.Stream`` or any
# object whose ``cuda_stream`` is a ``hipStream_t``; the variants that read a count or a total
# back (``out=None``; ``frames_scan`` unless ``read_count=False``) copy it on ``s`` and wait
# for ``s`` alone.

def _stream_handle(stream) -> int:
    t = _torch()
    s = stream if stream is not None else t.cuda.current_stream()
    return int(s.cuda_stream)


def _read_back(x, stream) -> int:
    """x[0] on the host, copied on the call's stream: that stream is synchronised, no other."""
    t = _torch()
    if stream is None:
        return int(x.cpu()[0])
    own = stream if isinstance(stream, t.cuda.Stream) else t.cuda.ExternalStream(int(stream.cuda_stream),
                                                                                 device=x.device)
    with t.cuda.stream(own):
        return int(x.cpu()[0])


def _dev_u32_out(n: int, device, out):
    t = _torch()
    if out is None:
        out = t.empty(n, dtype=t.int32, device=device)
    if out.numel() < n or out.element_size() != 4 or not out.is_contiguous():
        raise ValueError("out must be a contiguous 4-byte tensor with >= n elements")
    return out


def _ptr(x):
    """x's address for the C entry: NULL for None and for a tensor without elements."""
    return x.data_ptr() if x is not None and x.numel() else None


def _count(x) -> int:
    """x's element count for the C entry, 0 where ``_ptr(x)`` is NULL: a byte buffer's size."""
    return 0 if x is None else x.numel()
