// shade.hip — the shade kernels: every k_shade a scene's plan can name, and the BSDF probe's k_bsdf_eval, which makes k_shade's calls
// into device/bsdf.h.  (The units of the library: kernel_tables.h.)
#include <hip/hip_runtime.h>

#include "kernel_tables.h"

// The shade probe's sums (device/shade.h, PBRS_SHADE_MARK): defined here, once, beside every kernel that adds to them and the entry point that reads them.
#ifdef PBRS_PROBE_SHADE
__device__ unsigned long long g_shade_probe[16];
#define PBRS_SHADE_PROBE_DEFINED
#endif
#include "device/shade.h"
#include "device/bsdf_probe.h"

using namespace pbrs;

namespace {

// The k_shade instantiations (device/shade.h: INTEG, TEX, SPEC) the choices name: host/kernel_choice.h, PBRS_SHADE_KERNELS.
struct ShadeKernel {
    uint32_t integ;
    bool tex;
    uint32_t spec;
    shade_fn_t fn;
};
#define PBRS_SHADE_KERNEL_ENTRY(I, T, SP) ShadeKernel{I, T, SP, &k_shade<I, T, SP>},
const ShadeKernel kShadeKernels[] = {PBRS_SHADE_KERNELS(PBRS_SHADE_KERNEL_ENTRY)};
#undef PBRS_SHADE_KERNEL_ENTRY

}  // namespace

shade_fn_t pbrs::shade_fn(const ShadeKey& key) {
    for (const ShadeKernel& k : kShadeKernels)
        if (k.integ == key.integ && k.tex == key.tex && k.spec == key.spec) return k.fn;
    return nullptr;
}

bsdf_eval_fn_t pbrs::bsdf_eval_fn(bool lambert, bool fourier) {
    if (lambert) return fourier ? nullptr : &k_bsdf_eval<true, false>;
    return fourier ? &k_bsdf_eval<false, true> : &k_bsdf_eval<false, false>;
}

#ifdef PBRS_PROBE_SHADE
extern "C" {
// developer probe: reads and clears the k_shade region cycle sums
int pbrs_debug_shade_probe(unsigned long long* out16) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_shade_probe), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long zero[16] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_shade_probe), zero, sizeof zero) == hipSuccess ? 0 : -1;
}
}  // extern "C"
#endif
