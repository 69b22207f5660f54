// Opt-in bf16 inference convolution entry points (included by sepconv_capi.hip).

namespace {

// the instance of cbf16::conv_bf16<KS, MW, ACT> for the plan's wave layout (MW 4 or 2) and the activation
template <int KS>
decltype(&cbf16::conv_bf16<3, 4, 0>) bf16_kernel(int mw, int act) {
    if (mw == 4) return act == 0 ? cbf16::conv_bf16<KS, 4, 0> : act == 1 ? cbf16::conv_bf16<KS, 4, 1> : cbf16::conv_bf16<KS, 4, 2>;
    return act == 0 ? cbf16::conv_bf16<KS, 2, 0> : act == 1 ? cbf16::conv_bf16<KS, 2, 1> : cbf16::conv_bf16<KS, 2, 2>;
}

}  // namespace

extern "C" {

static int bf16_shape_ok(int K, int C, int k) { return C >= 16 && K >= 16 && (k == 3 || k == 5 || k == 7); }

long long tai_conv_bf16_weight_elems(int K, int C, int k) {
    g_err[0] = 0;
    if (!bf16_shape_ok(K, C, k)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16: needs C >= 16, K >= 16 and k in {3, 5, 7}");
    return (long long)((K + cbf16::NT - 1) / cbf16::NT) * ((C + cbf16::KC - 1) / cbf16::KC) * cbf16::ksteps(k) * (cbf16::STEP_BYTES / 2);
}

int tai_conv_bf16_pack_weights(const float* w, void* Wp, int K, int C, int k, int transposed, void* hip_stream) {
    g_err[0] = 0;
    if (!w || !Wp) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (!bf16_shape_ok(K, C, k)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_pack_weights: needs C >= 16, K >= 16 and k in {3, 5, 7}");
    if ((long long)K * C * k * k >= (1LL << 31)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_pack_weights: weight too large");
    if (!aligned(Wp, 16)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_pack_weights: Wp must be 16-byte aligned");
    const long long pairs = tai_conv_bf16_weight_elems(K, C, k) / 2;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(cbf16::pack_weights, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, w, static_cast<unsigned*>(Wp), K, C, k,
                       transposed ? 1 : 0, (C + cbf16::KC - 1) / cbf16::KC, pairs);
    return check_launch("conv_bf16_pack_weights");
}

// The plan of a launch as a query: the same cbf16::plan call and the same refusals (with the forward's words) as tai_conv_bf16_forward
// makes for N, K, H, W and k.  No stream, no launch.
int tai_conv_bf16_plan(int N, int K, int H, int W, int k, int* out) {
    g_err[0] = 0;
    if (!out) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (!bf16_shape_ok(K, 16, k)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: needs C >= 16, K >= 16 and k in {3, 5, 7}");
    if (N <= 0 || H <= 0 || W <= 0)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: needs N, H, W >= 1, C a multiple of the part count, act in {0, 1, 2}");
    if ((long long)N * K * H * W >= (1LL << 31))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: tensor too large (2^31 elements or more)");
    const cbf16::Plan pl = cbf16::plan(N, K, H, W, k);
    if (pl.blocks <= 0 || pl.blocks >= (1LL << 31)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: no tile fits");
    const int v[11] = {pl.MW, pl.TH, pl.TW, pl.IMG, pl.PH, pl.PW, pl.pitch, pl.tiles_x, pl.tiles_y, pl.groups, pl.lds_bytes};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
    return (int)pl.blocks;
}

int tai_conv_bf16_forward(const float* const* xs, int nparts, const void* Wp, const float* bias, float* y, float* ypool, const float* addx,
                          float* y2, int N, int C, int K, int H, int W, int k, int act, void* hip_stream) {
    g_err[0] = 0;
    if (!xs || !Wp || !bias || !y || nparts < 1 || nparts > 4) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: bad argument (1 to 4 input parts)");
    for (int p = 0; p < nparts; ++p)
        if (!xs[p]) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: null input part");
    if (!bf16_shape_ok(K, C, k)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: needs C >= 16, K >= 16 and k in {3, 5, 7}");
    if (N <= 0 || H <= 0 || W <= 0 || C % nparts != 0 || act < 0 || act > 2)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: needs N, H, W >= 1, C a multiple of the part count, act in {0, 1, 2}");
    if ((long long)N * C * H * W >= (1LL << 31) || (long long)N * K * H * W >= (1LL << 31))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: tensor too large (2^31 elements or more)");
    if ((ypool || addx) && (H % 2 != 0 || W % 2 != 0))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: the pool and unpool epilogues need even H and W");
    if (y2 && !addx) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: y2 needs addx");
    if (!aligned(Wp, 16)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: Wp must be 16-byte aligned");
    const cbf16::Plan pl = cbf16::plan(N, K, H, W, k);
    if (pl.blocks <= 0 || pl.blocks >= (1LL << 31)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_bf16_forward: no tile fits");
    cbf16::Args a{};
    for (int p = 0; p < 4; ++p) a.x[p] = xs[p < nparts ? p : 0];
    a.cpart = C / nparts;
    a.w = static_cast<const uint4*>(Wp);
    a.bias = bias; a.y = y; a.ypool = ypool; a.addx = addx; a.y2 = y2;
    a.N = N; a.C = C; a.K = K; a.H = H; a.W = W;
    a.TH = pl.TH; a.TW = pl.TW; a.IMG = pl.IMG; a.PH = pl.PH; a.PW = pl.PW; a.pitch = pl.pitch;
    a.tiles_x = pl.tiles_x; a.tiles_y = pl.tiles_y;
    a.kblocks = (K + cbf16::NT - 1) / cbf16::NT;
    a.nchunks = (C + cbf16::KC - 1) / cbf16::KC;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t lds = (size_t)pl.lds_bytes;
    auto kern = k == 3 ? bf16_kernel<3>(pl.MW, act) : k == 5 ? bf16_kernel<5>(pl.MW, act) : bf16_kernel<7>(pl.MW, act);
    if (int rc = launch(kern, dim3((unsigned)pl.blocks), dim3(cbf16::THREADS), lds, s, a)) return rc;
    return check_launch("conv_bf16_forward");
}

}  // extern "C"
