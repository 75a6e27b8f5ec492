"""Developer tools (GPU box): the HIP-event timing harness of tools/denoise_cost.py and tools/denoise_var_cost.py.  A Context on a
stream of its own, two events around what a function queues there, medians of repeated runs after a warm-up, and plain device buffers.
Import it after the package whose library is to be timed (it may be another checkout's)."""
import ctypes as C
import statistics


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


class Timing:
    def __init__(self, pbrs_amd, warmup, device=0):
        # the HIP runtime the library is linked against (already loaded with it); an older checkout's package has no api.hip_runtime
        pbrs_amd.gpu_lib()
        hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip = hip
        self.stream, self.ev0, self.ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(hip.hipStreamCreate(C.byref(self.stream)), "hipStreamCreate")
        check(hip.hipEventCreate(C.byref(self.ev0)), "hipEventCreate")
        check(hip.hipEventCreate(C.byref(self.ev1)), "hipEventCreate")
        self.warmup = warmup  # untimed runs before median_of's timed ones, unless it is told otherwise
        self.ctx = pbrs_amd.Context(device)
        self.ctx.set_stream(self.stream.value)

    def timed(self, fn):
        """Milliseconds of what fn queues on the context's stream."""
        hip = self.hip
        check(hip.hipEventRecord(self.ev0, self.stream), "hipEventRecord")
        fn()
        check(hip.hipEventRecord(self.ev1, self.stream), "hipEventRecord")
        check(hip.hipEventSynchronize(self.ev1), "hipEventSynchronize")
        ms = C.c_float()
        check(hip.hipEventElapsedTime(C.byref(ms), self.ev0, self.ev1), "hipEventElapsedTime")
        return float(ms.value)

    def median_of(self, fn, runs, warmup=None):
        for _ in range(self.warmup if warmup is None else warmup):
            self.timed(fn)
        ms = [round(self.timed(fn), 4) for _ in range(runs)]
        return {"ms": ms, "median_ms": round(statistics.median(ms), 4)}

    def dev_alloc(self, nbytes):
        ptr = C.c_void_p()
        check(self.hip.hipMalloc(C.byref(ptr), nbytes), "hipMalloc")
        return ptr
