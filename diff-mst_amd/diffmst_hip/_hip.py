"""Loader of the gfx950 kernel library.  Fails loudly: there is NO fallback path."""
from __future__ import annotations

import ctypes
import os

import torch

from . import _cabi

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# MST_HIP_LIB: developer override to load an A/B build of the same library (still no fallback)
LIB_PATH = os.environ.get("MST_HIP_LIB") or os.path.join(_PKG_ROOT, "lib", "libdiffmst_hip.so")
_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found - build it with `make -C diff-mst_amd/csrc` "
                "(hipcc --offload-arch=gfx950) or `python -c 'import __graft_entry__ as g; g.build()'`. "
                "The mst package has no CPU fallback."
            )
        _lib = _cabi.bind(ctypes.CDLL(LIB_PATH))
    return _lib


def current_stream_ptr(device) -> ctypes.c_void_p:
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # the raw handle without building a torch.cuda.Stream object (~10 us)
    if raw is not None:
        idx = device.index if getattr(device, "index", None) is not None else torch.cuda.current_device()
        return ctypes.c_void_p(raw(idx))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class launch_on:
    """``with launch_on(device) as stream: lib.mst_x(..., stream)``: the library launches on the current device, so ``device`` is made
    current for the call, and ``stream`` is the raw handle of torch's current stream on it.  (A class, not a generator: this runs once
    per kernel call.)"""

    __slots__ = ("device", "guard")

    def __init__(self, device):
        self.device, self.guard = device, torch.cuda.device(device)

    def __enter__(self) -> ctypes.c_void_p:
        self.guard.__enter__()
        return current_stream_ptr(self.device)

    def __exit__(self, *exc):
        return self.guard.__exit__(*exc)


def device_tables(cache: dict, key, device, tables_bytes, init_tables, *args, dtype=torch.float32, unsupported=None):
    """Constant tables of the kernels, built once per ``key`` (which names the device) and kept in ``cache``.  ``tables_bytes(*args)`` and
    ``init_tables(*args, tables, stream)`` are the library's pair for them; a size of 0 says that ``args`` are outside the kernels'
    limits and raises ``ValueError(unsupported)`` (pairs that take no configuration never return 0 and pass no message)."""
    t = cache.get(key)
    if t is None:
        nbytes = tables_bytes(*args)
        if nbytes == 0:
            raise ValueError(unsupported or f"{tables_bytes.__name__}{args} returned 0")
        t = torch.empty(nbytes // dtype.itemsize, dtype=dtype, device=device)
        with launch_on(device) as stream:
            init_tables(*args, t, stream)
        cache[key] = t
    return t


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "mst (MI355X build): tensors must live on a ROCm device (got a CPU tensor); "
                "there is no CPU path in this package"
            )


def require_same_device(device, *tensors):
    for t in tensors:
        if t is not None and t.device != device:
            raise RuntimeError(f"mst (MI355X build): every tensor of a call must live on {device} (got one on {t.device})")
