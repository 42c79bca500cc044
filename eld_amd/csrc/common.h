// common.h -- shared device/host helpers for libeld_amd (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/eld_amd.h"

#define ELD_WAVE 64

// Ablation switches (ELD_CONV_DBG / ELD_NOISE_DBG) and the s_memtime stage profiler (eld_debug_conv_prof) are DEVELOPER tools
// for tools/: they change numerical results by design.  Production builds compile them out (ELD_DEV_TOOLS=0, the default);
// build with HIPCC_EXTRA=-DELD_DEV_TOOLS=1 to get them back.
#ifndef ELD_DEV_TOOLS
#define ELD_DEV_TOOLS 0
#endif
#define ELD_DBG(a) (ELD_DEV_TOOLS ? (a).dbg : 0)
#define ELD_PROF(a) (ELD_DEV_TOOLS ? (a).prof : nullptr)

// Kernel launch: the per-thread "last error" of the HIP runtime is shared with every other user of the runtime in the process
// (PyTorch's own probes and event queries leave hipErrorNotReady / hipErrorNoDevice behind), so it is cleared right before
// the launch; ELD_LAUNCH_CHECK() after it then reports this launch only.
#define ELD_LAUNCH(...)                            \
    do {                                           \
        (void)hipGetLastError();                   \
        hipLaunchKernelGGL(__VA_ARGS__);           \
    } while (0)

#define ELD_LAUNCH_CHECK()                         \
    do {                                           \
        hipError_t e__ = hipGetLastError();        \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

// unsigned division by a launch-uniform divisor without the ~30-instruction udiv expansion
struct FastDiv {
    uint32_t d, m, s;
};

static inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d ? d : 1;
    uint32_t l = 0;
    while ((1ull << l) < f.d) ++l;
    f.s = l;
    f.m = (uint32_t)(((1ull << 32) * ((1ull << l) - f.d)) / f.d + 1);
    return f;
}

__device__ __forceinline__ uint32_t fdiv_u32(uint32_t n, FastDiv f) {
    return (uint32_t)(((uint64_t)__umulhi(n, f.m) + n) >> f.s);
}

static inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }

// Test hook behind eld_debug_last_conv_kernel: the launcher that picks a convolution or weight-gradient kernel family records its name (a
// string literal) right before the launch.  Host-side only: one relaxed atomic store per launch, no device work.
void eld_note_conv_kernel(const char* family);
// A launcher that runs a NON-default variant of its family (an ELD_* switch of this process chose another instantiation or another tile shape) records
// "family/v1[,v2[,v3]]" instead: v1..v3 are string literals naming what differs from the default (nullptr or "": nothing), so a switch that is no
// longer read or no longer reaches its kernel shows in the name.  With every part empty this is eld_note_conv_kernel(family): default runs keep
// their names.  The joined names are interned once per distinct name (a mutex, non-default runs only).
void eld_note_conv_variant(const char* family, const char* v1, const char* v2 = nullptr, const char* v3 = nullptr);

// compute units of the CURRENT device (persistent-grid sizing); read once per device, immutable afterwards
static inline int eld_num_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        hipDeviceProp_t p;
        int n = (hipGetDeviceProperties(&p, dev) == hipSuccess) ? p.multiProcessorCount : 0;
        cus[dev] = n > 0 ? n : 256;
    }
    return cus[dev];
}

// workgroups of a grid-stride pass over `units` lanes' worth of work: at most 8 per compute unit
static inline unsigned stride_grid(uint32_t units, int threads) {
    const long long nb = ((long long)units + threads - 1) / threads, cap = 8ll * eld_num_cus();
    return (unsigned)(nb < cap ? nb : cap);
}

// a mosaic the 8-columns-per-lane passes (shading.hip, flatfield.hip) refuse: odd width, or more sites than a 32-bit unit count holds
static inline bool bad_shape(int Hm, int Wm) { return Hm < 0 || Wm < 0 || Wm % 2 || (uint64_t)Hm * (uint64_t)Wm >= (1ull << 31); }

// a Bayer raw_pattern (4 ints, not null): a permutation of the colour codes 0..3.  Each caller builds its own table from it.
static inline bool bayer_permutation(const int* raw_pattern) {
    unsigned seen = 0u;
    for (int i = 0; i < 4; ++i) {
        if (raw_pattern[i] < 0 || raw_pattern[i] > 3) return false;
        seen |= 1u << raw_pattern[i];
    }
    return seen == 15u;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remember which devices a kernel has been prepared on
struct EldAttrOnce {
    bool done[64] = {false};
    template <typename K>
    int ensure(K kern, size_t lds_bytes) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        if (!done[dev]) {
            hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return (int)e;
            done[dev] = true;
        }
        return 0;
    }
};
