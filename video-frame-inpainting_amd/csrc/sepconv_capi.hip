// C ABI of the MI355X-native adaptive separable convolution (see include/tai_sepconv.h).
//
// Replaces the reference's cffi-exported shim SeparableConvolution_cuda_forward / _backward
// (src/separable_convolution/cfile/SeparableConvolution_cuda.c:8-25, :28-51) and its launchers
// (SeparableConvolution_kernel.cu:164-185, :187-242).  gfx950 only; no host synchronisation,
// allocation or copy on any path, so every call can be captured into a hipGraph.
//
// One translation unit: the kernels (*.hip.inc), the host helpers every launcher shares (below), then the entry points, one
// capi_<family>.inc per kernel family (the includes at the end of this file).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_set>

#include "tai_sepconv.h"

#include "sepconv_fwd.hip.inc"
#include "sepconv_bwd.hip.inc"
#include "upsample.hip.inc"
#include "bias_act.hip.inc"
#include "thin_conv.hip.inc"
#include "wino_conv.hip.inc"
#include "wino_split.hip.inc"
#include "wino43_conv.hip.inc"
#include "wino_wrw.hip.inc"
#include "conv_bf16.hip.inc"
#include "spectral_norm.hip.inc"
#include "hbm_probe.hip.inc"
#include "frame_metrics.hip.inc"
#include "ssim_loss.hip.inc"
#include "image_loss.hip.inc"
#include "lap_loss.hip.inc"
#include "temporal_loss.hip.inc"
#include "census_loss.hip.inc"
#include "clip_pipeline.hip.inc"
#include "clip_augment.hip.inc"
#include "frame_scan.hip.inc"
#include "block_scan.hip.inc"
#include "damage_composite.hip.inc"
#include "state_digest.hip.inc"
#include "grad_stats.hip.inc"
#include "fused_step.hip.inc"

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char* fmt, const char* what) {
    std::snprintf(g_err, sizeof(g_err), fmt, what);
    return code;
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        std::snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
        return TAI_SEPCONV_ELAUNCH;
    }
    return TAI_SEPCONV_OK;
}

// Raises the kernel's dynamic-LDS limit past the default 64 KiB.  The attribute is per DEVICE and sticks, so it is set
// once per (device, kernel, size) and remembered only after the runtime accepted it: the steady-state launch path makes
// no runtime call besides hipGetDevice and the launch itself.
template <typename KernelT>
int allow_lds(KernelT kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return TAI_SEPCONV_OK;
    constexpr int SLOTS = 64;
    static thread_local const void* done_kernel[SLOTS];
    static thread_local size_t done_bytes[SLOTS];
    static thread_local int done_device[SLOTS];
    static thread_local int n_done = 0;
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess) return fail(TAI_SEPCONV_ELAUNCH, "%s", "hipGetDevice");
    const void* key = reinterpret_cast<const void*>(kernel);
    for (int i = 0; i < n_done; ++i)
        if (done_kernel[i] == key && done_device[i] == device && done_bytes[i] >= bytes) return TAI_SEPCONV_OK;
    const hipError_t e = hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        std::snprintf(g_err, sizeof(g_err), "hipFuncSetAttribute(lds=%zu): %s", bytes, hipGetErrorString(e));
        return TAI_SEPCONV_ELAUNCH;
    }
    if (n_done < SLOTS) { done_kernel[n_done] = key; done_bytes[n_done] = bytes; done_device[n_done] = device; ++n_done; }
    return TAI_SEPCONV_OK;
}

// compute units of the current device (cached per device and thread, like allow_lds: no runtime call on the launch path after
// the first)
static int device_cu_count() {
    static thread_local int cached_device = -1, cached_cus = 0;
    int device = -1;
    if (hipGetDevice(&device) != hipSuccess) return 0;
    if (device != cached_device) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
        cached_device = device; cached_cus = n;
    }
    return cached_cus;
}

// One launch: the LDS limit raised where the kernel asks for more than 64 KiB (allow_lds, whose code this returns), then the
// kernel.  The caller asks check_launch() when it wants the launch's own error.  All instantiations of a kernel template share
// a signature, so a launcher picks the instance into a plain function pointer and comes here once.
template <typename... P, typename... A>
int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args) {
    if (int rc = allow_lds(kern, lds)) return rc;
    hipLaunchKernelGGL(kern, grid, block, lds, s, static_cast<P>(args)...);
    return TAI_SEPCONV_OK;
}

// workgroups of 256 threads over `work` items, at most `cap` (the kernels stride by the whole grid)
int grid_for(long long work, int cap) {
    const long long blocks = (work + 255) / 256;
    return (int)(blocks < cap ? blocks : cap);
}

bool aligned(const void* p, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

// dynamic LDS of the forward's row-loop kernels and of the kernels that share their loops: a patch of (rows + 50) x 180 floats
// rounded up to 1 KiB, then the tap ring, TAI_FWD_ROWLOOP_RING_SLOTS KiB per wave
size_t rowloop_lds(int rows, int waves, size_t extra = 0) {
    const size_t patch = (size_t)(rows + 50) * 180 * sizeof(float);
    return ((patch + 1023) & ~(size_t)1023) + (size_t)waves * TAI_FWD_ROWLOOP_RING_SLOTS * 1024 + extra;
}

// A divisor of the Winograd kernels' index arithmetic as a multiply-high constant (wino::DivMagic):
// n / d == (n * m) >> (32 + s) for every n < 2^31: s = floor(log2 d), one less for a power of two (m = 2^31, exact); for any
// other d, 2^s < d gives m = ceil(2^(32+s) / d) < 2^32 and an error term e = m d - 2^(32+s) < d, so n e < 2^(32+s) holds for
// n <= 2^(32+s) / d, which exceeds 2^31.  d == 1 is flagged by m == 0.
void wino_div_magic(long long d, unsigned& m, unsigned& sh) {
    if (d <= 1) { m = 0; sh = 0; return; }
    int lg = 0;
    while ((2LL << lg) <= d) ++lg;                          // floor(log2 d)
    if ((1LL << lg) == d) --lg;
    sh = (unsigned)lg;
    const unsigned __int128 num = (unsigned __int128)1 << (32 + lg);
    m = (unsigned)((num + (unsigned __int128)d - 1) / (unsigned __int128)d);
}

}  // namespace

extern "C" {

int tai_sepconv_version(void) { return 890; }

const char* tai_sepconv_last_error(void) { return g_err; }

#ifndef TAI_SOURCE_HASH
#define TAI_SOURCE_HASH "unknown"
#endif
// -DTAI_SOURCE_HASH="..." from _native.build().  The marker in front lets the loader read the hash from the FILE, without mapping
// a binary it may be about to refuse (and without dlopen's by-name cache handing back a library that was since rebuilt).
static const char k_source_hash[] = "TAI_SOURCE_HASH=" TAI_SOURCE_HASH;
const char* tai_sepconv_source_hash(void) { return k_source_hash + 16; }

}  // extern "C"

#include "capi_sepconv.inc"
#include "capi_pointwise.inc"
#include "capi_wino43.inc"
#include "capi_wino.inc"
#include "capi_bf16.inc"
#include "capi_image.inc"
#include "capi_scan.inc"
#include "capi_tables.inc"
