// Adaptive separable convolution: forward and backward launchers (included by sepconv_capi.hip).

namespace {

// Kernel selectors (benchmarking / tests).  Process-wide; relaxed atomics so a selector flipped by one thread while
// another launches is a defined (if unordered) read, never a torn one.
std::atomic<int> g_fwd_variant{0};
std::atomic<int> g_gi_variant{0};   // 0 automatic, 1 force the gather kernel
std::atomic<int> g_vh_variant{0};   // 0 automatic (fused asm kernel for C == 1 when both gradients are wanted), 1 HIP kernels

bool dims_ok(int B, int C, int H, int W, int ks) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || ks <= 0) return false;
    const long long lim = 0x7fffffffLL;
    const long long Hp = H + ks - 1, Wp = W + ks - 1;
    return (long long)B * C * Hp * Wp < lim && (long long)B * ks * H * W < lim;
}

template <int KS, int NC, int SPLIT>
int launch_fwd_tiled(const float* in, const float* v, const float* h, float* out, int B, int C, int c0,
                     int H, int W, hipStream_t s) {
    using K = fwd::Cfg<KS, SPLIT>;
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W;
    const int tiles_y = (H + K::TILE_H - 1) / K::TILE_H;
    const size_t lds = K::lds_bytes(NC);
    if (int rc = launch(fwd::sepconv_forward_tiled<KS, NC, SPLIT>, dim3(B * tiles_x * tiles_y), dim3(K::THREADS), lds, s, in, v, h, out,
                        C, c0, H, W, tiles_x, tiles_y))
        return rc;
    return check_launch("sepconv_forward_tiled");
}

template <int KS, int NC>
int launch_fwd_packed(const float* in, const float* v, const float* h, float* out, int B, int C, int c0,
                      int H, int W, hipStream_t s) {
    using K = fwd::Cfg<KS, 1>;
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W;
    const int tiles_y = (H + K::TILE_H - 1) / K::TILE_H;
    const size_t lds = K::lds_bytes(NC);
    if (int rc = launch(fwd::sepconv_forward_packed<KS, NC>, dim3(B * tiles_x * tiles_y), dim3(K::THREADS), lds, s, in, v, h, out, C, c0,
                        H, W, tiles_x, tiles_y))
        return rc;
    return check_launch("sepconv_forward_packed");
}

template <bool STAGGER, int DBG = 0, int WAVES = 4, int ASMV = 0>
int fwd_asm_all_channels(const float* in, const float* v, const float* h, float* out, int B, int C, int H,
                         int W, hipStream_t s) {
    constexpr int TILE_H = 2 * WAVES;
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W;
    const int tiles_y = (H + TILE_H - 1) / TILE_H;
    const size_t lds = rowloop_lds(TILE_H, WAVES);
    auto kern = fwd::sepconv_forward_asm<STAGGER, DBG, WAVES, ASMV>;
    if (int rc = allow_lds(kern, lds)) return rc;
    for (int c0 = 0; c0 < C; ++c0) {
        hipLaunchKernelGGL(kern, dim3(B * tiles_x * tiles_y), dim3(WAVES * 64), lds, s, in, v, h, out, C, c0, H, W,
                           tiles_x, tiles_y);
        if (int rc = check_launch("sepconv_forward_asm")) return rc;
    }
    return TAI_SEPCONV_OK;
}

template <int MIXMODE, int DBG = 0>
int fwd_ab_all_channels(const float* in, const float* v, const float* h, float* out, int B, int C, int H, int W,
                        hipStream_t s) {
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W;
    const int tiles_y = (H + 15) / 16;
    const size_t lds = rowloop_lds(16, 8, MIXMODE == 5 ? 16 : 0);
    auto kern = fwd::sepconv_forward_ab<MIXMODE, DBG>;
    if (int rc = allow_lds(kern, lds)) return rc;
    for (int c0 = 0; c0 < C; ++c0) {
        hipLaunchKernelGGL(kern, dim3(B * tiles_x * tiles_y), dim3(512), lds, s, in, v, h, out, C, c0, H, W, tiles_x,
                           tiles_y);
        if (int rc = check_launch("sepconv_forward_ab")) return rc;
    }
    return TAI_SEPCONV_OK;
}

// kernel 20: one persistent workgroup per CU over the tiles of a single-channel frame batch; kernel 18 runs instead when there
// is at most one tile per CU (nothing to overlap) or the tile count is not a multiple of 8 (the XCD-contiguous tile order)
// POLICY: 0 = by footprint (nt loads and the reversed tile walk when the two tap tensors together exceed the Infinity Cache:
// every tap byte is read once and none of it will be there for anybody else), 1 = default cache policy, forward walk (round 3's
// kernel 20), 2 = nt, forward walk, 3 = nt, reversed walk, 4 = default cache policy, reversed walk, 5 / 6 / 7 = as 3 with the
// type-A waves at constant priority 0 / 1 / 2.
// THE decision (forward_route below, and through it tai_sepconv_forward and tai_sepconv_forward_route): the concrete policy 1-7
// the persistent kernel runs with on the current device, or 0 when the launch goes to kernel 18.
int persistent_policy(int B, int C, int H, int W, bool force, int policy) {
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W, tiles_y = (H + 15) / 16;
    const int ntiles = B * tiles_x * tiles_y;
    const int cus = device_cu_count();
    const int grid = cus > 0 ? (cus / 8) * 8 : 0;
    if (C != 1 || grid < 8 || ntiles % 8 != 0 || (!force && ntiles <= grid) || (long long)B * 51 * H * W * 4 > 0xffffffffLL)
        return 0;
    if (policy == 0) policy = (2LL * B * 51 * H * W * 4 > (256LL << 20)) ? 6 : 1;
    return policy;
}

// the persistent launch itself, with a concrete policy from persistent_policy (which has checked C == 1, the tile count and the
// 32-bit tap offsets)
template <int DBG = 0>
int launch_persistent(const float* in, const float* v, const float* h, float* out, int B, int H, int W, hipStream_t s, int policy) {
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W, tiles_y = (H + 15) / 16;
    const int ntiles = B * tiles_x * tiles_y;
    const int cus = device_cu_count();
    int grid = cus > 0 ? (cus / 8) * 8 : 0;
    if (grid > ntiles) grid = ntiles;
    const size_t lds = rowloop_lds(16, 8, 16) + rowloop_lds(16, 0);       // (a second patch: the next tile's, staged behind this one's rows)
    // <DBG, NT, REV, APRIO>: nt tap loads, reversed tile walk, priority of the type-A waves (-1: as their partners')
    auto kern = fwd::sepconv_forward_persistent<DBG, false, false, -1>;
    if (policy == 5) kern = fwd::sepconv_forward_persistent<DBG, true, true, 0>;
    else if (policy == 6) kern = fwd::sepconv_forward_persistent<DBG, true, true, 1>;
    else if (policy == 7) kern = fwd::sepconv_forward_persistent<DBG, true, true, 2>;
    else if (policy == 3) kern = fwd::sepconv_forward_persistent<DBG, true, true, -1>;
    else if (policy == 4) kern = fwd::sepconv_forward_persistent<DBG, false, true, -1>;
    else if (policy == 2) kern = fwd::sepconv_forward_persistent<DBG, true, false, -1>;
    if (int rc = launch(kern, dim3(grid), dim3(512), lds, s, in, v, h, out, H, W, tiles_x, tiles_y, ntiles)) return rc;
    return check_launch("sepconv_forward_persistent");
}

#ifdef TAI_TIMING_VARIANTS
// the persistent kernel with time stamps (tools build): forced, same decision, kernel 18 (without stamps) where it does not run
int fwd_persistent_stamped(const float* in, const float* v, const float* h, float* out, int B, int C, int H, int W, hipStream_t s,
                           int policy) {
    const int p = persistent_policy(B, C, H, W, true, policy);
    return p ? launch_persistent<1>(in, v, h, out, B, H, W, s, p) : fwd_ab_all_channels<5>(in, v, h, out, B, C, H, W, s);
}
#endif

// What tai_sepconv_forward runs for a REQUESTED variant (0 = automatic) on the current device: the variant number of the kernel
// of the leading channels, or a negative error code with the message set.  tai_sepconv_forward switches on this value and
// tai_sepconv_forward_route returns it: there is no second copy of these conditions.
int forward_route(int B, int C, int H, int W, int ks, int requested) {
    if (!dims_ok(B, C, H, W, ks)) return fail(TAI_SEPCONV_EINVAL, "%s", "bad dimensions");
    const bool tileable = (ks == 51) && (W % 4 == 0);
    // default: mixed type-A / type-B hand-scheduled kernel for single-channel frames; three channel patches per tap row otherwise
    const int variant = requested == 0 ? tai_sepconv_default_forward_variant(C, W, ks) : requested;
    if (variant != 1 && !tileable)
        return fail(TAI_SEPCONV_EINVAL, "%s", "tiled forward variants need ks == 51 and W % 4 == 0");
    if (variant >= 20 && variant <= 27) {
        // 20: by footprint, persistent at any tile count only when asked for by number; 21-27: that policy, at any tile count
        const int policy = persistent_policy(B, C, H, W, requested != 0, variant - 20);
        return policy ? 20 + policy : 18;
    }
    if (variant == 17 || variant == 19) return C >= 3 ? variant : 16;      // no channel triple: every channel on kernel 16
    const bool known = (variant >= 1 && variant <= 16) || variant == 18;
#ifdef TAI_TIMING_VARIANTS
    if (variant >= 101 && variant <= 127) return variant;                   // (the switch refuses the numbers that do not exist)
#endif
    if (!known) return fail(TAI_SEPCONV_EINVAL, "%s", "unknown forward variant (values >= 100 exist only in the tools build, -DTAI_TIMING_VARIANTS)");
    return variant;
}

template <int WAVES>
int fwd_asm_channel_loop(const float* in, const float* v, const float* h, float* out, int B, int C, int H, int W,
                          hipStream_t s) {
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W;
    const int tiles_y = (H + 2 * WAVES - 1) / (2 * WAVES);
    if (int rc = launch(fwd::sepconv_forward_asm_channels<WAVES>, dim3(B * tiles_x * tiles_y), dim3(WAVES * 64), rowloop_lds(2 * WAVES, WAVES), s,
                        in, v, h, out, C, H, W, tiles_x, tiles_y))
        return rc;
    return check_launch("sepconv_forward_asm_channels");
}

// channels in groups of three through the three-patch row loop; what is left over through the per-channel loop
template <bool EARLY, int ABL = 0>
int fwd_asm_three_channels(const float* in, const float* v, const float* h, float* out, int B, int C, int H, int W, hipStream_t s) {
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W, tiles_y = (H + 15) / 16;
    const size_t lds = (size_t)3 * TAI_FWD_ROWLOOP_C3_PATCH_BYTES + (size_t)8 * TAI_FWD_ROWLOOP_C3_RING_SLOTS * 1024;
    auto kern = fwd::sepconv_forward_asm_c3<EARLY, ABL>;
    if (int rc = allow_lds(kern, lds)) return rc;
    int c0 = 0;
    for (; c0 + 3 <= C; c0 += 3) {
        hipLaunchKernelGGL(kern, dim3(B * tiles_x * tiles_y), dim3(512), lds, s, in, v, h, out, C, c0, H, W, tiles_x, tiles_y);
        if (int rc = check_launch("sepconv_forward_asm_c3")) return rc;
    }
    for (; c0 < C; ++c0) {
        // (kernel 16: its LDS size has no counter word)
        if (int rc = launch(fwd::sepconv_forward_ab<4, 0>, dim3(B * tiles_x * tiles_y), dim3(512), rowloop_lds(16, 8), s, in, v, h, out, C, c0, H, W,
                            tiles_x, tiles_y))
            return rc;
        if (int rc = check_launch("sepconv_forward_ab")) return rc;
    }
    return TAI_SEPCONV_OK;
}

template <int KS>
int fwd_packed_all_channels(const float* in, const float* v, const float* h, float* out, int B, int C,
                            int H, int W, hipStream_t s) {
    int c0 = 0;
    for (; c0 + 3 <= C; c0 += 3)
        if (int rc = launch_fwd_packed<KS, 3>(in, v, h, out, B, C, c0, H, W, s)) return rc;
    for (; c0 < C; ++c0)
        if (int rc = launch_fwd_packed<KS, 1>(in, v, h, out, B, C, c0, H, W, s)) return rc;
    return TAI_SEPCONV_OK;
}

template <int KS, int SPLIT>
int fwd_tiled_all_channels(const float* in, const float* v, const float* h, float* out, int B, int C,
                           int H, int W, hipStream_t s) {
    int c0 = 0;
    for (; c0 + 3 <= C; c0 += 3)
        if (int rc = launch_fwd_tiled<KS, 3, SPLIT>(in, v, h, out, B, C, c0, H, W, s)) return rc;
    for (; c0 < C; ++c0)
        if (int rc = launch_fwd_tiled<KS, 1, SPLIT>(in, v, h, out, B, C, c0, H, W, s)) return rc;
    return TAI_SEPCONV_OK;
}

template <int KS, int NC>
int launch_grad_vh_tiled(const float* gO, const float* in, const float* v, const float* h, float* gV,
                         float* gH, int B, int H, int W, hipStream_t s) {
    using K = fwd::Cfg<KS, 1>;
    const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W;
    const int tiles_y = (H + K::TILE_H - 1) / K::TILE_H;
    const size_t lds = K::lds_bytes(NC);
    const dim3 grid(B * tiles_x * tiles_y), block(K::THREADS);
    if (gV) {
        if (int rc = launch(bwd::sepconv_grad_v_tiled<KS, NC>, grid, block, lds, s, gO, in, h, gV, H, W, tiles_x, tiles_y)) return rc;
        if (int rc = check_launch("sepconv_grad_v_tiled")) return rc;
    }
    if (gH) {
        if (int rc = launch(bwd::sepconv_grad_h_tiled<KS, NC>, grid, block, lds, s, gO, in, v, gH, H, W, tiles_x, tiles_y)) return rc;
        if (int rc = check_launch("sepconv_grad_h_tiled")) return rc;
    }
    return TAI_SEPCONV_OK;
}

}  // namespace

extern "C" {

int tai_sepconv_set_forward_variant(int variant) { return g_fwd_variant.exchange(variant, std::memory_order_relaxed); }

int tai_sepconv_set_grad_taps_variant(int variant) { return g_vh_variant.exchange(variant, std::memory_order_relaxed); }

int tai_sepconv_set_grad_input_variant(int variant) { return g_gi_variant.exchange(variant, std::memory_order_relaxed); }

int tai_sepconv_default_forward_variant(int C, int W, int ks) {
    const bool tileable = (ks == 51) && (W % 4 == 0);
    return !tileable ? 1 : (C == 1 ? 20 : 19);
}

int tai_sepconv_forward_route(int B, int C, int H, int W, int ks, int variant) {
    g_err[0] = 0;
    return forward_route(B, C, H, W, ks, variant);
}

long long tai_sepconv_forward_bytes(int B, int C, int H, int W, int ks) {
    const long long Hp = H + ks - 1, Wp = W + ks - 1;
    return 4LL * ((long long)B * C * Hp * Wp + 2LL * B * ks * H * W + (long long)B * C * H * W);
}

long long tai_sepconv_backward_bytes(int B, int C, int H, int W, int ks) {
    const long long Hp = H + ks - 1, Wp = W + ks - 1;
    return 4LL * ((long long)B * C * H * W + 2LL * B * C * Hp * Wp + 4LL * B * ks * H * W);
}

int tai_sepconv_forward(const float* input, const float* vertical, const float* horizontal,
                        float* output, int B, int C, int H, int W, int ks, void* hip_stream) {
    g_err[0] = 0;
    if (!input || !vertical || !horizontal || !output) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    // the kernel this launch runs: decided in one place, which tai_sepconv_forward_route reports
    const int route = forward_route(B, C, H, W, ks, g_fwd_variant.load(std::memory_order_relaxed));
    if (route < 0) return route;
    switch (route) {
        case 1: {
            const int n = B * C * H * W;
            hipLaunchKernelGGL(fwd::sepconv_forward_generic, dim3((n + 255) / 256), dim3(256), 0, s, input,
                               vertical, horizontal, output, n, C, H, W, ks);
            return check_launch("sepconv_forward_generic");
        }
        case 2: return fwd_tiled_all_channels<51, 1>(input, vertical, horizontal, output, B, C, H, W, s);
        case 3: return fwd_tiled_all_channels<51, 2>(input, vertical, horizontal, output, B, C, H, W, s);
        case 4: return fwd_packed_all_channels<51>(input, vertical, horizontal, output, B, C, H, W, s);
        case 5: return fwd_asm_all_channels<false>(input, vertical, horizontal, output, B, C, H, W, s);
        case 6: return fwd_asm_all_channels<true>(input, vertical, horizontal, output, B, C, H, W, s);
        case 7: return fwd_asm_all_channels<false, 0, 8>(input, vertical, horizontal, output, B, C, H, W, s);
        case 8: return fwd_asm_all_channels<true, 0, 8>(input, vertical, horizontal, output, B, C, H, W, s);
        case 9: return fwd_asm_all_channels<false, 0, 8, 1>(input, vertical, horizontal, output, B, C, H, W, s);
        case 10: return fwd_ab_all_channels<0>(input, vertical, horizontal, output, B, C, H, W, s);
        case 11: return fwd_ab_all_channels<1>(input, vertical, horizontal, output, B, C, H, W, s);
        case 12: return fwd_ab_all_channels<2>(input, vertical, horizontal, output, B, C, H, W, s);
        case 13: return fwd_ab_all_channels<3>(input, vertical, horizontal, output, B, C, H, W, s);
        case 16: return fwd_ab_all_channels<4>(input, vertical, horizontal, output, B, C, H, W, s);
        case 18: return fwd_ab_all_channels<5>(input, vertical, horizontal, output, B, C, H, W, s);
        case 14: return fwd_asm_channel_loop<8>(input, vertical, horizontal, output, B, C, H, W, s);
        case 15: return fwd_asm_channel_loop<4>(input, vertical, horizontal, output, B, C, H, W, s);
        case 17: return fwd_asm_three_channels<false>(input, vertical, horizontal, output, B, C, H, W, s);
        case 19: return fwd_asm_three_channels<true>(input, vertical, horizontal, output, B, C, H, W, s);
        // (20 itself never arrives here: forward_route resolves it to its policy, 21 or 26 by footprint, or to kernel 18)
        case 21:        // default cache policy, forward walk
        case 22:        // A/B: nt tap loads, forward walk
        case 23:        // A/B: nt tap loads, reversed walk
        case 24:        // A/B: default cache policy, reversed walk
        case 25:        // A/B: as 23, type A at constant priority 0
        case 26:        // as 23, type A at constant priority 1
        case 27:        // A/B: as 23, type A at constant priority 2
            return launch_persistent(input, vertical, horizontal, output, B, H, W, s, route - 20);
#ifdef TAI_TIMING_VARIANTS   // timing experiments (wrong results by design): tools/ build only, never in the shipped library
        case 117: return fwd_asm_three_channels<true, 1>(input, vertical, horizontal, output, B, C, H, W, s);   // kernel 19 without the v-ring wait
        case 118: return fwd_asm_three_channels<true, 2>(input, vertical, horizontal, output, B, C, H, W, s);   // kernel 19 without the window waits
        case 108: return fwd_ab_all_channels<3, 3>(input, vertical, horizontal, output, B, C, H, W, s);
        case 109: return fwd_ab_all_channels<4, 3>(input, vertical, horizontal, output, B, C, H, W, s);   // kernel 16 with stamps
        case 110: return fwd_ab_all_channels<5, 3>(input, vertical, horizontal, output, B, C, H, W, s);   // kernel 18 with stamps
        case 120: return fwd_persistent_stamped(input, vertical, horizontal, output, B, C, H, W, s, 0);    // kernel 20 with stamps
        case 123: return fwd_persistent_stamped(input, vertical, horizontal, output, B, C, H, W, s, 3);  // 23 (round 4's first scheme) with stamps
        case 125: return fwd_persistent_stamped(input, vertical, horizontal, output, B, C, H, W, s, 5);  // 25 / 26 / 27 with stamps
        case 126: return fwd_persistent_stamped(input, vertical, horizontal, output, B, C, H, W, s, 6);
        case 127: return fwd_persistent_stamped(input, vertical, horizontal, output, B, C, H, W, s, 7);
        case 106: return fwd_ab_all_channels<0, 3>(input, vertical, horizontal, output, B, C, H, W, s);
        case 107: return fwd_ab_all_channels<2, 3>(input, vertical, horizontal, output, B, C, H, W, s);
        case 111: return fwd_asm_all_channels<false, 0, 8, 2>(input, vertical, horizontal, output, B, C, H, W, s);
        case 112: return fwd_asm_all_channels<false, 0, 8, 3>(input, vertical, horizontal, output, B, C, H, W, s);
        case 103: return fwd_asm_all_channels<false, 3, 8>(input, vertical, horizontal, output, B, C, H, W, s);
        case 104: return fwd_asm_all_channels<true, 3, 8>(input, vertical, horizontal, output, B, C, H, W, s);
        case 105: return fwd_asm_all_channels<false, 3, 4>(input, vertical, horizontal, output, B, C, H, W, s);
        case 101: return fwd_asm_all_channels<false, 1>(input, vertical, horizontal, output, B, C, H, W, s);
        case 102: return fwd_asm_all_channels<false, 2>(input, vertical, horizontal, output, B, C, H, W, s);
#endif
        default: return fail(TAI_SEPCONV_EINVAL, "%s", "unknown forward variant (values >= 100 exist only in the tools build, -DTAI_TIMING_VARIANTS)");
    }
}

int tai_sepconv_backward(const float* grad_output, const float* input, const float* vertical,
                         const float* horizontal, float* grad_input, float* grad_vertical,
                         float* grad_horizontal, int B, int C, int H, int W, int ks, void* hip_stream) {
    g_err[0] = 0;
    if (!grad_output || !input || !vertical || !horizontal) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (!dims_ok(B, C, H, W, ks)) return fail(TAI_SEPCONV_EINVAL, "%s", "bad dimensions");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);

    const bool tileable = (ks == 51) && (W % 4 == 0) && (C == 1 || C == 3);
    const int gi_variant = g_gi_variant.load(std::memory_order_relaxed);
    bool gi_done = false;
    if (grad_input && tileable && (gi_variant == 0 || gi_variant == 3 || gi_variant == 4)) {
        // gI FIRST (the reference launches V, H, I -- SeparableConvolution_kernel.cu:201-239 -- but the three are
        // independent): wave-private accumulation strips; the tile slabs go to the caller's grad_vertical (or
        // grad_horizontal) buffer, which is filled only afterwards, and a second kernel sums them in a fixed order.
        const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W, tiles_y = (H + bwd::gi2::R - 1) / bwd::gi2::R;
        const long long slab_bytes = (long long)B * tiles_x * tiles_y * C * bwd::gi2::SLAB * (long long)sizeof(float);
        float* scratch = grad_vertical ? grad_vertical : grad_horizontal;
        // A slab is gi2::SLAB = 10,800 floats per tile and channel against 51 H W floats of tap gradient per sample: small planes
        // (below ~212 pixels per tile and channel, e.g. [1,1,2,104] or [1,3,5,124]) do not hold them and flush with atomics instead.
        if (slab_bytes > (long long)B * ks * H * W * (long long)sizeof(float)) scratch = nullptr;
        const size_t lds = (size_t)bwd::gi2::LDS_FLOATS * sizeof(float);
        const dim3 grid(B * tiles_x * tiles_y), block(512);
        float* dst = scratch ? scratch : grad_input;
        if (!scratch) {      // no buffer to borrow: float atomics on a zeroed gI (last bits then depend on arrival order)
            const size_t bytes = (size_t)B * C * (H + ks - 1) * (W + ks - 1) * sizeof(float);
            if (hipMemsetAsync(grad_input, 0, bytes, s) != hipSuccess) return fail(TAI_SEPCONV_ELAUNCH, "%s", "hipMemsetAsync(gI)");
        }
        const bool use_asm = gi_variant != 4;                  // 4: the HIP C++ row loop (A/B)
        const int to_scratch = scratch ? 1 : 0;
        auto kern = C == 1 ? (use_asm ? bwd::sepconv_grad_i_strips_asm<1> : bwd::sepconv_grad_i_strips<1>)
                           : (use_asm ? bwd::sepconv_grad_i_strips_asm<3> : bwd::sepconv_grad_i_strips<3>);
        if (int rc = launch(kern, grid, block, lds, s, grad_output, vertical, horizontal, dst, H, W, tiles_x, tiles_y, to_scratch)) return rc;
        if (int rc = check_launch("sepconv_grad_i_strips")) return rc;
        if (scratch) {
            const int n = B * C * (H + ks - 1) * ((W + ks - 1) / 2);
            hipLaunchKernelGGL(bwd::sepconv_grad_i_reduce, dim3((n + 255) / 256), dim3(256), 0, s, scratch, grad_input, n, C, H, W,
                               tiles_x, tiles_y, use_asm ? 2 : 0);
            if (int rc = check_launch("sepconv_grad_i_reduce")) return rc;
        }
        gi_done = true;
    }

    const int vh_variant = g_vh_variant.load(std::memory_order_relaxed);
    if (tileable && C == 1 && (grad_vertical || grad_horizontal) && vh_variant != 1) {
        // the tap gradients of a single-channel frame in one launch of the hand-scheduled wave types; requested alone, a gradient
        // runs on the same waves (the other four leave early), so its bits do not depend on what else was asked for
        const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W, tiles_y = (H + 7) / 8;
        // default: gV waves at their gH partners' priority: 112-114 -> 109.6 us at [32,1,128,128], 490 -> 487 at [160,...] (same process)
        auto kern = bwd::sepconv_grad_vh_ab<true, 1>;
        // (variant 2: the round-2 form that stages the patch behind a workgroup barrier before the tap loads; A/B and tests)
        if (vh_variant == 2) kern = bwd::sepconv_grad_vh_ab<false>;
        else if (vh_variant == 3) kern = bwd::sepconv_grad_vh_ab<true, 0>;      // A/B: gV waves left at priority 0 (the default until round 4)
        else if (vh_variant == 4) kern = bwd::sepconv_grad_vh_ab<true, 2>;      // A/B: gV waves at priority 2
        if (int rc = launch(kern, dim3(B * tiles_x * tiles_y), dim3(512), rowloop_lds(8, 8), s, grad_output, input, vertical, horizontal,
                            grad_vertical, grad_horizontal, H, W, tiles_x, tiles_y))
            return rc;
        if (int rc = check_launch("sepconv_grad_vh_ab")) return rc;
    } else if (tileable) {
        const int rc = (C == 1) ? launch_grad_vh_tiled<51, 1>(grad_output, input, vertical, horizontal,
                                                                grad_vertical, grad_horizontal, B, H, W, s)
                                : launch_grad_vh_tiled<51, 3>(grad_output, input, vertical, horizontal,
                                                                grad_vertical, grad_horizontal, B, H, W, s);
        if (rc) return rc;
    } else {
        const int n = B * ks * H * W;
        if (grad_vertical) {
            hipLaunchKernelGGL(bwd::sepconv_grad_v_generic, dim3((n + 255) / 256), dim3(256), 0, s,
                               grad_output, input, horizontal, grad_vertical, n, C, H, W, ks);
            if (int rc = check_launch("sepconv_grad_v_generic")) return rc;
        }
        if (grad_horizontal) {
            hipLaunchKernelGGL(bwd::sepconv_grad_h_generic, dim3((n + 255) / 256), dim3(256), 0, s,
                               grad_output, input, vertical, grad_horizontal, n, C, H, W, ks);
            if (int rc = check_launch("sepconv_grad_h_generic")) return rc;
        }
    }
    if (grad_input && !gi_done) {
        if (tileable && gi_variant == 2) {
            // first form: LDS row-scatter with a barrier per tap row; accumulates into gI with atomics, so zero it first
            const size_t bytes = (size_t)B * C * (H + ks - 1) * (W + ks - 1) * sizeof(float);
            if (hipMemsetAsync(grad_input, 0, bytes, s) != hipSuccess) return fail(TAI_SEPCONV_ELAUNCH, "%s", "hipMemsetAsync(gI)");
            const int tiles_x = (W + fwd::TILE_W - 1) / fwd::TILE_W, tiles_y = (H + 7) / 8;
            const dim3 grid(B * tiles_x * tiles_y), block(512);
            const size_t lds = ((size_t)C * 58 * 180 + 8 * 2 * 320) * sizeof(float);
            auto kern = C == 1 ? bwd::sepconv_grad_i_rows<51, 1> : bwd::sepconv_grad_i_rows<51, 3>;
            if (int rc = launch(kern, grid, block, lds, s, grad_output, vertical, horizontal, grad_input, H, W, tiles_x, tiles_y)) return rc;
            if (int rc = check_launch("sepconv_grad_i_rows")) return rc;
            return TAI_SEPCONV_OK;
        }
        const int n = B * (H + ks - 1) * (W + ks - 1);
        const dim3 grid((n + 255) / 256), block(256);
        int c0 = 0;
        for (; c0 + 3 <= C; c0 += 3) {
            hipLaunchKernelGGL(bwd::sepconv_grad_i_gather<3>, grid, block, 0, s, grad_output, vertical,
                               horizontal, grad_input, n, C, c0, H, W, ks);
            if (int rc = check_launch("sepconv_grad_i_gather<3>")) return rc;
        }
        for (; c0 < C; ++c0) {
            hipLaunchKernelGGL(bwd::sepconv_grad_i_gather<1>, grid, block, 0, s, grad_output, vertical,
                               horizontal, grad_input, n, C, c0, H, W, ks);
            if (int rc = check_launch("sepconv_grad_i_gather<1>")) return rc;
        }
    }
    return TAI_SEPCONV_OK;
}

}  // extern "C"
