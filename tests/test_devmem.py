"""pbrs_amd.devmem.DeviceBuffers against a stub of the HIP runtime that records every call: what is freed, how often, and what is
raised, without a GPU."""
import numpy as np
import pytest

from pbrs_amd import PbrsError
from pbrs_amd.devmem import DEVICE_TO_HOST, HOST_TO_DEVICE, DeviceBuffers


class StubHip:
    """hipMalloc hands out 0x1000, 0x2000, ...; `fail_malloc`: the 1-based allocation that fails; `fail_copy`: every hipMemcpy fails."""

    def __init__(self, fail_malloc=None, fail_copy=False):
        self.calls, self.fail_malloc, self.fail_copy, self.mallocs = [], fail_malloc, fail_copy, 0

    def hipMalloc(self, ref, nbytes):
        self.mallocs += 1
        if self.mallocs == self.fail_malloc:
            self.calls.append(("hipMalloc", None, nbytes))
            return 2
        ref._obj.value = 0x1000 * self.mallocs
        self.calls.append(("hipMalloc", ref._obj.value, nbytes))
        return 0

    def hipMemcpy(self, dst, src, nbytes, kind):
        self.calls.append(("hipMemcpy", nbytes, kind))
        return 1 if self.fail_copy else 0

    def hipFree(self, ptr):
        self.calls.append(("hipFree", ptr.value))
        return 0

    def freed(self):
        return [c[1] for c in self.calls if c[0] == "hipFree"]


SIZES = {"a": 16, "b": 32, "c": 48, "d": 64, "e": 80}


def test_a_failing_allocation_frees_the_earlier_ones_once_each():
    hip = StubHip(fail_malloc=3)
    buf = DeviceBuffers.__new__(DeviceBuffers)
    with pytest.raises(PbrsError, match="hipMalloc of 48 bytes for a test failed"):
        buf.__init__(SIZES, "a test", hip=hip)
    assert hip.freed() == [0x1000, 0x2000] and hip.mallocs == 3
    assert len(buf) == 0 and buf.ptrs() == {}
    buf.free()
    assert hip.freed() == [0x1000, 0x2000]


def test_with_frees_each_pointer_exactly_once_also_when_the_body_raises():
    for boom in (False, True):
        hip = StubHip()
        try:
            with DeviceBuffers(SIZES, "a test", hip=hip) as buf:
                assert buf["b"].value == 0x2000 and buf.ptr("c") == 0x3000 and buf.ptr(None) is None
                assert buf.ptrs(("e", "a")) == {"e": 0x5000, "a": 0x1000} and len(buf) == 5
                if boom:
                    raise KeyError("the body's own")
        except KeyError:
            assert boom
        assert sorted(hip.freed()) == [0x1000, 0x2000, 0x3000, 0x4000, 0x5000]
        buf.free()  # a second free() does nothing
        assert len(hip.freed()) == 5 and len(buf) == 0


def test_arrays_are_allocated_and_uploaded():
    hip = StubHip()
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    with DeviceBuffers({"a": a, "n": 8}, hip=hip) as buf:
        assert hip.calls == [("hipMalloc", 0x1000, 24), ("hipMemcpy", 24, HOST_TO_DEVICE), ("hipMalloc", 0x2000, 8)]
        got = buf.download_like("a", a)
        assert got.shape == a.shape and got.dtype == a.dtype and got is not a and hip.calls[-1] == ("hipMemcpy", 24, DEVICE_TO_HOST)
        assert buf.download("n", (2,), np.uint32).shape == (2,)
    assert (HOST_TO_DEVICE, DEVICE_TO_HOST) == (1, 2)  # hipMemcpyKind


def test_an_upload_of_the_wrong_size_raises_before_any_copy():
    hip = StubHip()
    with DeviceBuffers({"a": 24}, hip=hip) as buf:
        n = len(hip.calls)
        with pytest.raises(ValueError, match="20 bytes for a, which holds 24"):
            buf.upload("a", np.zeros(5, dtype=np.float32))
        with pytest.raises(ValueError):
            buf.download("a", (7,), np.float32)
        assert len(hip.calls) == n
        buf.upload("a", np.zeros(6, dtype=np.float32))
        assert hip.calls[n:] == [("hipMemcpy", 24, HOST_TO_DEVICE)]


def test_a_failing_copy_raises_pbrs_error():
    hip = StubHip(fail_copy=True)
    with DeviceBuffers({"a": 24}, "a test", hip=hip) as buf:
        with pytest.raises(PbrsError, match="hipMemcpy of a of a test failed"):
            buf.download("a", (2, 3), np.float32)
        with pytest.raises(PbrsError, match="hipMemcpy of the image failed"):
            buf.download("a", (2, 3), np.float32, "the image")
        with pytest.raises(PbrsError, match="hipMemcpy"):
            buf.upload("a", np.zeros(6, dtype=np.float32))
    with pytest.raises(PbrsError, match="hipMemcpy"):  # the upload of the array form: its allocation is freed
        DeviceBuffers({"a": np.zeros(6, dtype=np.float32)}, hip=hip)
    assert hip.freed() == [0x1000, 0x2000]


@pytest.mark.gpu
def test_a_round_trip_on_the_real_runtime(gpu_ctx):
    rng = np.random.default_rng(3)
    arrays = {"f": rng.normal(size=(5, 7, 3)).astype(np.float32), "u": rng.integers(0, 1 << 32, size=(5, 7), dtype=np.uint32),
              "b": rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)}
    arrays["f"][0, 0] = [np.nan, np.inf, -0.0]
    buf = DeviceBuffers(arrays, "a round trip")
    assert len(buf) == 3 and all(buf.ptr(n) for n in arrays) and buf["u"].value == buf.ptr("u")
    for n, a in arrays.items():
        got = buf.download_like(n, a)
        assert got is not a and got.dtype == a.dtype and got.tobytes() == a.tobytes(), n
    buf.upload("u", arrays["u"][::-1])  # (not contiguous as given)
    assert buf.download("u", (5, 7), np.uint32).tobytes() == arrays["u"][::-1].tobytes()
    assert buf.download("b", (7, 4), np.uint8).tobytes() == arrays["b"][0].tobytes()  # the start of a plane
    buf.free()
    buf.free()
    assert len(buf) == 0
