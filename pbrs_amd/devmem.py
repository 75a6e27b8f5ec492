"""Device memory of the driver's chains and of the tests: one owner for a set of named allocations."""
import ctypes as C

import numpy as np

from .libs import PbrsError, hip_runtime

HOST_TO_DEVICE, DEVICE_TO_HOST = 1, 2  # hipMemcpyKind


class DeviceBuffers:
    """Named device allocations made through the HIP runtime (`hip`: what stands in for libs.hip_runtime()), from {name: nbytes} or
    from {name: ndarray}, which also uploads the array.  `what` names their purpose in messages.  A context manager; free() releases
    every pointer once, however often it is called, and hipFree is the only synchronisation on the way out.  If an allocation fails
    the earlier ones are freed before PbrsError is raised."""

    def __init__(self, sizes, what="device buffers", hip=None):
        self._ptrs, self._nbytes = {}, {}
        self._hip = hip_runtime() if hip is None else hip
        self.what = what
        try:
            for name, size in sizes.items():
                nbytes = size.nbytes if isinstance(size, np.ndarray) else int(size)
                ptr = C.c_void_p()
                if self._hip.hipMalloc(C.byref(ptr), nbytes) != 0:
                    raise PbrsError(f"hipMalloc of {nbytes} bytes for {what} failed")
                self._ptrs[name], self._nbytes[name] = ptr, nbytes
                if isinstance(size, np.ndarray):
                    self.upload(name, size)
        except BaseException:
            self.free()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def free(self):
        ptrs, self._ptrs, self._nbytes = self._ptrs, {}, {}
        for ptr in ptrs.values():
            self._hip.hipFree(ptr)

    def __getitem__(self, name):
        return self._ptrs[name]

    def __len__(self):
        return len(self._ptrs)

    def ptr(self, name):
        """The address as an int; None for None (an optional plane that is not there)."""
        return None if name is None else self._ptrs[name].value

    def ptrs(self, names=None):
        """{name: address} of `names` (None: all)."""
        return {n: self._ptrs[n].value for n in (self._ptrs if names is None else names)}

    def _copy(self, dst, src, nbytes, kind, what):
        if self._hip.hipMemcpy(dst, src, nbytes, kind) != 0:
            raise PbrsError(f"hipMemcpy of {what} failed")

    def upload(self, name, array):
        a = np.ascontiguousarray(array)
        if a.nbytes != self._nbytes[name]:
            raise ValueError(f"{a.nbytes} bytes for {name}, which holds {self._nbytes[name]}")
        self._copy(self._ptrs[name], a.ctypes.data, a.nbytes, HOST_TO_DEVICE, f"{name} to the device")

    def download(self, name, shape, dtype, what=None):
        """A fresh array of `shape` and `dtype` from the start of `name`; `what`: the failure's message names it instead of `name`."""
        out = np.empty(shape, dtype=dtype)
        if out.nbytes > self._nbytes[name]:
            raise ValueError(f"{out.nbytes} bytes from {name}, which holds {self._nbytes[name]}")
        self._copy(out.ctypes.data, self._ptrs[name], out.nbytes, DEVICE_TO_HOST, what or f"{name} of {self.what}")
        return out

    def download_like(self, name, array, what=None):
        return self.download(name, array.shape, array.dtype, what)
