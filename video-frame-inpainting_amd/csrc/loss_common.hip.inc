// What the metric and loss kernels share (frame_metrics, ssim_loss, image_loss, lap_loss, temporal_loss; each includes this file
// itself): force-inlined device helpers only, so a kernel's code is what it was with the helper written out in its own file.
#pragma once

namespace losscommon {

// the sum over the wave's 64 lanes, in every lane: a butterfly, the same order whatever the lane
template <typename V>
__device__ __forceinline__ V wave_sum(V x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// util.inverse_transform in fp32, not clipped
__device__ __forceinline__ float range_map(float v) {
#pragma clang fp contract(off)
    return (v + 1.f) / 2.f;
}

// sgn(0) = 0, NaN kept
__device__ __forceinline__ float sgn(float v) {
    return v != v ? v : (float)((v > 0.f) - (v < 0.f));
}

// rho(d) and rho'(d) of kind 0 (L2: d * d, 2 * d), 1 (L1: |d|, sgn(d)) and 2 (Charbonnier: sqrt(d * d + e2), d / that), every fp32
// operation as written
__device__ __forceinline__ void rho_drho(int kind, float d, float e2, float& rho, float& drho) {
#pragma clang fp contract(off)
    if (kind == 0) {
        rho = d * d;
        drho = 2.f * d;
    } else if (kind == 1) {
        rho = __builtin_fabsf(d);
        drho = sgn(d);
    } else {
        rho = __builtin_sqrtf(d * d + e2);
        drho = d / rho;
    }
}

}  // namespace losscommon
