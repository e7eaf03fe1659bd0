"""The one marshalling layer between the package's Python and libtaco_hip: tensor / lengths (inputs onto the device, shape checks),
workspace (a handle's scratch memory), buffers (result tensors kept per shape), device_of, call (device, stream, pointers, status)
and Handle (a library handle with its close / __del__ pair).  PyTorch holds the memory and the streams; nothing here computes."""
import ctypes as C

import numpy as np
import torch

from . import _lib

STREAM = object()       # in call's arguments: the place of the current stream


def pointer(t):
    """A tensor's address, NULL for None"""
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    """The current stream of the current device"""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def tensor(x, device, dtype, what, dims=None):
    """numpy or tensor -> a contiguous `dtype` tensor on the device (one that already is that is used as it is).  dtype may be a tuple:
    the input's own if it is among them, else the first.  dims: per dimension its name (any size) or (name, size); None: the caller
    checks the shape."""
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if isinstance(dtype, tuple):
        dtype = x.dtype if x.dtype in dtype else dtype[0]
    x = x.to(device, dtype).contiguous()
    if dims is not None and (x.dim() != len(dims) or any(not isinstance(d, str) and x.shape[i] != d[1] for i, d in enumerate(dims))):
        raise Exception("%s must be [%s], got shape %s" % (what, ", ".join(d if isinstance(d, str) else "%s = %d" % d for d in dims), tuple(x.shape)))
    return x


def lengths(v, device, B, what):
    """The optional [B] int32 vector (frames, num_samples): a device int32 tensor is used as it is, host data is uploaded, None stays None."""
    return None if v is None else tensor(v, device, torch.int32, what, (("B", B),))


def device_of(*xs):
    """The device of the first CUDA tensor among xs, else the current CUDA device"""
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda:%d" % torch.cuda.current_device())


def workspace(handle, nbytes):
    """The handle's workspace, grown to nbytes"""
    if handle._ws is None or handle._ws.numel() < nbytes:
        handle._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=handle.device)
    return handle._ws


def buffers(cache, key, **specs):
    """The buffer set cache[key] (key[0] names its device), made or extended to hold every name of specs = (shape, dtype).  A tensor
    that is in the set is never replaced: a later call of the same key gets the same storage, which keeps captured graphs valid."""
    buf = cache.setdefault(key, {})
    for name, (shape, dtype) in specs.items():
        if name not in buf:
            buf[name] = torch.empty(shape, dtype=dtype, device=key[0])
    return buf


def _arg(a):
    if a is STREAM:
        return stream()
    if a is None or torch.is_tensor(a):
        return pointer(a)
    return a


def call(device, fn, *args):
    """fn(*args) on the device's current stream (where args holds STREAM): tensors and None go as pointers, the status is checked.
    device None: no device context is entered (a plan launch, a stage call: the caller's current device and stream are the ones)."""
    if device is None:
        _lib.check(fn(*[_arg(a) for a in args]))
    else:
        with torch.cuda.device(device):
            _lib.check(fn(*[_arg(a) for a in args]))


class Handle(object):
    """A library handle, kept in the attribute named `_handle_attr` and released by the library function named `_destroy`."""
    _destroy = None
    _handle_attr = "_h"

    def close(self):
        if getattr(self, self._handle_attr, None):
            getattr(self._lib, self._destroy)(getattr(self, self._handle_attr))
            setattr(self, self._handle_attr, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
