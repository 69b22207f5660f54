// What the metric and loss kernels share (frame_metrics, ssim_loss, image_loss, lap_loss, temporal_loss, census_loss; each includes this
// file itself): force-inlined device helpers, so a kernel's code is what it was with the helper written out in its own file, and one host
// check (block_strides_fault) of the two launchers that read [B, T, C, H, W] tensors where they lie.
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

// One tensor's batch and time strides (temporal_loss, census_loss): 0 when they are positive, every element's offset is below 2^40 and no
// two of the B x T blocks of chw elements overlap; else which of the three fails.  Two blocks overlap when |db * sb + dt * st| < chw for
// some (db, dt) != (0, 0): for every db of the shorter axis the dt nearest to -db * sb / st is looked at (the distance is monotone in dt
// on either side of it).
enum { STRIDES_OK = 0, STRIDES_NOT_POSITIVE, STRIDES_REACH_2_40, STRIDES_OVERLAP };

inline int block_strides_fault(long long sb, long long st, int B, int T, long long chw) {
    if (sb < 1 || st < 1) return STRIDES_NOT_POSITIVE;
    const long long lim = 1LL << 40;
    if (sb >= lim || st >= lim || (B > 1 && sb > (lim - chw) / (B - 1)) || (T > 1 && st > (lim - chw) / (T - 1)) ||
        (long long)(B - 1) * sb + (long long)(T - 1) * st + chw > lim)
        return STRIDES_REACH_2_40;
    long long sa = sb, so = st;            // sa: the stride of the shorter axis, looped over
    int na = B, no = T;
    if (T < B) { sa = st; so = sb; na = T; no = B; }
    for (long long da = 0; da < na; ++da) {
        const long long base = da * sa;    // < 2^40
        long long k = -(base / so);        // the multiples of `so` on either side of -base
        for (int side = 0; side < 2; ++side, --k) {
            long long dt = k;
            if (dt < -(long long)(no - 1)) dt = -(long long)(no - 1);
            if (dt > (long long)(no - 1)) dt = (long long)(no - 1);
            if (da == 0 && dt == 0) continue;
            const long long dist = base + dt * so;
            if ((dist < 0 ? -dist : dist) < chw) return STRIDES_OVERLAP;
        }
    }
    return STRIDES_OK;
}

}  // namespace losscommon
