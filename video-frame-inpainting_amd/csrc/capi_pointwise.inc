// Pointwise and thin-layer entry points (included by sepconv_capi.hip).

extern "C" {

int tai_hbm_read_probe(const void* buffer, long long bytes, int nt, float* sink, void* hip_stream) {
    g_err[0] = 0;
    if (!buffer || !sink || bytes < (1 << 20)) return fail(TAI_SEPCONV_EINVAL, "%s", "hbm_read_probe: needs a buffer of at least 1 MiB and a sink of 4096 floats");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t n4 = (size_t)bytes / 16;
    hipLaunchKernelGGL(nt ? probe::stream_read<true> : probe::stream_read<false>, dim3(4096), dim3(256), 0, s,
                       static_cast<const probe::f4v*>(buffer), sink, n4);
    return check_launch("hbm_read_probe");
}

int tai_bias_act_inplace(float* x, const float* bias, int N, int C, int HW, int act, void* hip_stream) {
    g_err[0] = 0;
    if (!x || !bias) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || C <= 0 || HW <= 0 || act < 0 || act > 2) return fail(TAI_SEPCONV_EINVAL, "%s", "bad dimensions or activation");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const long long n = (long long)N * C * HW;
    const bool vec = (HW % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
    const long long work = vec ? n / 4 : n;
    const int blocks = grid_for(work, 16384);
    if (vec) {
        auto kern = act == bact::ACT_RELU ? bact::bias_act_vec4<bact::ACT_RELU>
                  : act == bact::ACT_TANH ? bact::bias_act_vec4<bact::ACT_TANH> : bact::bias_act_vec4<bact::ACT_NONE>;
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, x, bias, n / 4, HW / 4, C);
    } else {
        auto kern = act == bact::ACT_RELU ? bact::bias_act_scalar<bact::ACT_RELU>
                  : act == bact::ACT_TANH ? bact::bias_act_scalar<bact::ACT_TANH> : bact::bias_act_scalar<bact::ACT_NONE>;
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, x, bias, n, HW, C);
    }
    return check_launch("bias_act");
}

int tai_conv_cin1_forward(const float* x, const float* weight, const float* bias, float* y, int N, int Co, int H, int W,
                          int k, int act, void* hip_stream) {
    g_err[0] = 0;
    if (!x || !weight || !bias || !y) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || Co <= 0 || H <= 0 || W <= 0 || W % 4 != 0 || (k != 3 && k != 5) || act < 0 || act > 1)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_cin1: needs W % 4 == 0, k in {3, 5}, act in {0, 1}");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const long long work = (long long)N * H * (W / 4);
    const int blocks = grid_for(work, 8192);
    const int cgroups = (work < 4 * 262144 && Co >= 16) ? 4 : 1;      // few waves: split the output channels over gridDim.y
    auto kern = k == 3 ? (act == 0 ? thin::conv_cin1<3, 0> : thin::conv_cin1<3, 1>) : (act == 0 ? thin::conv_cin1<5, 0> : thin::conv_cin1<5, 1>);
    hipLaunchKernelGGL(kern, dim3(blocks, cgroups), dim3(256), 0, s, x, weight, bias, y, N, Co, H, W);
    return check_launch("conv_cin1");
}

int tai_conv_cin1_forward_maxpool_window(const float* x, const float* weight, const float* bias, float* y, float* ypool, int N,
                                         int Co, int H, int W, int k, int act, int pool_h, int pool_w, int pool_oy, int pool_ox,
                                         void* hip_stream) {
    g_err[0] = 0;
    if (!x || !weight || !bias || !y || !ypool) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || Co <= 0 || H <= 0 || W <= 0 || W % 4 != 0 || H % 2 != 0 || (k != 3 && k != 5) || act < 0 || act > 1)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_cin1_maxpool: needs W % 4 == 0, even H, k in {3, 5}, act in {0, 1}");
    if (pool_oy < 0 || pool_ox < 0 || pool_h < H / 2 + pool_oy || pool_w < W / 2 + pool_ox)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_cin1_maxpool: bad pooled-output window");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const long long work = (long long)N * (H / 2) * (W / 4);
    const int blocks = grid_for(work, 8192);
    const int cgroups = (work < 4 * 262144 && Co >= 16) ? 4 : 1;
    auto kern = k == 3 ? (act == 0 ? thin::conv_cin1_pool<3, 0> : thin::conv_cin1_pool<3, 1>)
                       : (act == 0 ? thin::conv_cin1_pool<5, 0> : thin::conv_cin1_pool<5, 1>);
    hipLaunchKernelGGL(kern, dim3(blocks, cgroups), dim3(256), 0, s, x, weight, bias, y, ypool, N, Co, H, W, pool_h, pool_w, pool_oy, pool_ox);
    return check_launch("conv_cin1_maxpool");
}

int tai_conv_cin1_forward_maxpool(const float* x, const float* weight, const float* bias, float* y, float* ypool, int N, int Co,
                                  int H, int W, int k, int act, void* hip_stream) {
    return tai_conv_cin1_forward_maxpool_window(x, weight, bias, y, ypool, N, Co, H, W, k, act, H / 2, W / 2, 0, 0, hip_stream);
}

int tai_unpool2x_add(const float* x, const float* res, float* out, long long planes, int h, int w, void* hip_stream) {
    g_err[0] = 0;
    if (!x || !res || !out) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (planes <= 0 || h <= 0 || w <= 0 || w % 2 != 0) return fail(TAI_SEPCONV_EINVAL, "%s", "unpool2x_add: needs even w");
    const long long work = planes * 2 * h * (2 * w / 4);
    const int blocks = grid_for(work, 16384);
    hipLaunchKernelGGL(bact::unpool2x_add, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), x, res, out, planes, h, w);
    return check_launch("unpool2x_add");
}

int tai_convlstm_gates_forward(const float* gates, const float* c, float* new_c, float* new_h, int N, int F, int HW,
                               float forget_bias, void* hip_stream) {
    g_err[0] = 0;
    if (!gates || !c || !new_c || !new_h) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || F <= 0 || HW <= 0 || HW % 4 != 0) return fail(TAI_SEPCONV_EINVAL, "%s", "convlstm_gates: needs HW % 4 == 0");
    const long long work = (long long)N * F * (HW / 4);
    const int blocks = grid_for(work, 16384);
    hipLaunchKernelGGL(bact::convlstm_gates, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), gates, c, new_c,
                       new_h, N, F, HW / 4, forget_bias);
    return check_launch("convlstm_gates");
}

int tai_sn_power_iteration(float* weight, float* u, float* scratch, float* sigma_out, int out_rows, int in_cols, int Ip,
                           void* hip_stream) {
    g_err[0] = 0;
    if (!weight || !u || !scratch) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (out_rows <= 0 || in_cols <= 0 || Ip <= 0 || Ip > 64) return fail(TAI_SEPCONV_EINVAL, "%s", "sn_power_iteration: bad shape or Ip");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    float* v_raw = scratch;
    float* t_raw = scratch + in_cols;
    float* sigma = sigma_out;
    const dim3 wt_block(snorm::WT_COLS, snorm::WT_ROWGROUPS);
    const int wt_grid = (in_cols + snorm::WT_COLS - 1) / snorm::WT_COLS;
    for (int it = 0; it < Ip; ++it) {
        // the stored u is used as it is (SNDiscriminator.py:20-22); later rounds consume the unnormalised product t_raw
        hipLaunchKernelGGL(snorm::wt_u, dim3(wt_grid), wt_block, 0, stream, weight, it == 0 ? u : t_raw, v_raw, out_rows, in_cols,
                           it == 0 ? 0 : 1);
        hipLaunchKernelGGL(snorm::w_v, dim3(out_rows), dim3(256), 0, stream, weight, v_raw, t_raw, in_cols);
    }
    const long long n = (long long)out_rows * in_cols;
    const long long want = (n / 4 + 255) / 256;
    const int blocks = (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
    hipLaunchKernelGGL(snorm::finish, dim3(blocks), dim3(256), 0, stream, weight, t_raw, u, sigma, out_rows, n);
    return check_launch("sn_power_iteration");
}

int tai_window_scale_bias_lrelu(float* y, const float* bias, const float* inv_scale, int nw, int B, int C, int HW, float slope,
                                void* hip_stream) {
    g_err[0] = 0;
    if (!y || !bias || !inv_scale) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (nw <= 0 || B <= 0 || C <= 0 || HW <= 0 || HW % 4 != 0) return fail(TAI_SEPCONV_EINVAL, "%s", "window_scale_bias_lrelu: needs HW % 4 == 0");
    const long long n4 = (long long)nw * B * C * (HW / 4);
    const int blocks = grid_for(n4, 16384);
    hipLaunchKernelGGL(snorm::window_scale_bias_lrelu, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), y, bias,
                       inv_scale, n4, C * (HW / 4), HW / 4, C, B, slope);
    return check_launch("window_scale_bias_lrelu");
}

int tai_window_scale_lrelu_backward(const float* grad_y, const float* y, const float* inv_scale, float* grad_z, float* grad_scaled,
                                    int nw, int B, int C, int HW, float slope, void* hip_stream) {
    g_err[0] = 0;
    if (!grad_y || !y || !inv_scale || !grad_z || !grad_scaled) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (nw <= 0 || B <= 0 || C <= 0 || HW <= 0 || HW % 4 != 0) return fail(TAI_SEPCONV_EINVAL, "%s", "window_scale_lrelu_backward: needs HW % 4 == 0");
    const long long n4 = (long long)nw * B * C * (HW / 4);
    const int blocks = grid_for(n4, 16384);
    hipLaunchKernelGGL(snorm::window_scale_lrelu_backward, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), grad_y, y,
                       inv_scale, grad_z, grad_scaled, n4, C * (HW / 4), B, slope);
    return check_launch("window_scale_lrelu_backward");
}

// The same two passes on any plane, one element per thread (a 4-element group would straddle two channels where HW % 4 != 0)
int tai_window_scale_bias_lrelu_scalar(float* y, const float* bias, const float* inv_scale, int nw, int B, int C, int HW, float slope,
                                       void* hip_stream) {
    g_err[0] = 0;
    if (!y || !bias || !inv_scale) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (nw <= 0 || B <= 0 || C <= 0 || HW <= 0 || (long long)nw * B * C >= (1LL << 31))
        return fail(TAI_SEPCONV_EINVAL, "%s", "window_scale_bias_lrelu_scalar: bad dimensions");
    const int planes = nw * B * C;
    const int blocks = planes < 16384 ? planes : 16384;
    hipLaunchKernelGGL(snorm::window_scale_bias_lrelu_scalar, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), y, bias,
                       inv_scale, planes, HW, C, B, slope);
    return check_launch("window_scale_bias_lrelu_scalar");
}

int tai_window_scale_lrelu_backward_scalar(const float* grad_y, const float* y, const float* inv_scale, float* grad_z, float* grad_scaled,
                                           int nw, int B, int C, int HW, float slope, void* hip_stream) {
    g_err[0] = 0;
    if (!grad_y || !y || !inv_scale || !grad_z || !grad_scaled) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (nw <= 0 || B <= 0 || C <= 0 || HW <= 0 || (long long)nw * B * C >= (1LL << 31))
        return fail(TAI_SEPCONV_EINVAL, "%s", "window_scale_lrelu_backward_scalar: bad dimensions");
    const int planes = nw * B * C;
    const int blocks = planes < 16384 ? planes : 16384;
    hipLaunchKernelGGL(snorm::window_scale_lrelu_backward_scalar, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), grad_y,
                       y, inv_scale, grad_z, grad_scaled, planes, HW, C, B, slope);
    return check_launch("window_scale_lrelu_backward_scalar");
}

int tai_thin_conv_wrw(const float* big, const float* thin, float* dw, float* dbias, float* workspace, int N, int Cb, int H, int W,
                      int k, void* hip_stream) {
    g_err[0] = 0;
    if (!big || !thin || !workspace || (!dw && !dbias)) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || Cb <= 0 || H <= 0 || W <= 0 || W % 4 != 0 || (k != 3 && k != 5) || (long long)N * Cb > 0x7fffffffLL)
        return fail(TAI_SEPCONV_EINVAL, "%s", "thin_conv_wrw: needs W % 4 == 0 and k in {3, 5}");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(k == 3 ? thin::thin_wrw<3> : thin::thin_wrw<5>, dim3(N * Cb), dim3(256), 0, stream, big, thin, workspace, N, Cb, H, W);
    if (int rc = check_launch("thin_conv_wrw")) return rc;
    const int total = Cb * (k * k + 1);
    hipLaunchKernelGGL(thin::thin_wrw_reduce, dim3((total + 255) / 256), dim3(256), 0, stream, workspace, dw, dbias, N, Cb, k * k);
    return check_launch("thin_conv_wrw_reduce");
}

int tai_act_maxpool2x2_forward(const float* z, float* y, float* ypool, long long planes, int H, int W, int relu, void* hip_stream) {
    g_err[0] = 0;
    if (!z || !y || !ypool) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (planes <= 0 || H <= 0 || W <= 0 || H % 2 != 0 || W % 4 != 0) return fail(TAI_SEPCONV_EINVAL, "%s", "act_maxpool2x2: needs even H and W % 4 == 0");
    const long long work = planes * (H / 2) * (W / 4);
    const int blocks = grid_for(work, 16384);
    hipLaunchKernelGGL(bact::act_pool2x2_forward, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), z, y, ypool, planes,
                       H, W, relu ? 1 : 0);
    return check_launch("act_maxpool2x2_forward");
}

int tai_act_maxpool2x2_backward(const float* grad_y, const float* grad_ypool, const float* y, float* grad_z, long long planes, int H,
                                int W, int relu, void* hip_stream) {
    g_err[0] = 0;
    if (!y || !grad_z) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (planes <= 0 || H <= 0 || W <= 0 || H % 2 != 0 || W % 4 != 0) return fail(TAI_SEPCONV_EINVAL, "%s", "act_maxpool2x2: needs even H and W % 4 == 0");
    const long long work = planes * (H / 2) * (W / 4);
    const int blocks = grid_for(work, 16384);
    hipLaunchKernelGGL(bact::act_pool2x2_backward, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), grad_y, grad_ypool,
                       y, grad_z, planes, H, W, relu ? 1 : 0);
    return check_launch("act_maxpool2x2_backward");
}

int tai_convlstm_gates_backward(const float* gates, const float* c, const float* new_c, const float* grad_new_c,
                                const float* grad_new_h, float* grad_gates, float* grad_c, int N, int F, int HW, float forget_bias,
                                void* hip_stream) {
    g_err[0] = 0;
    if (!gates || !c || !new_c || !grad_gates || !grad_c || (!grad_new_c && !grad_new_h)) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || F <= 0 || HW <= 0 || HW % 4 != 0) return fail(TAI_SEPCONV_EINVAL, "%s", "convlstm_gates: needs HW % 4 == 0");
    const long long work = (long long)N * F * (HW / 4);
    const int blocks = grid_for(work, 16384);
    hipLaunchKernelGGL(bact::convlstm_gates_backward, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), gates, c,
                       new_c, grad_new_c, grad_new_h, grad_gates, grad_c, N, F, HW / 4, forget_bias);
    return check_launch("convlstm_gates_backward");
}

int tai_conv_shift_stack(const float* x, float* out, int N, int C, int H, int W, int k, void* hip_stream) {
    g_err[0] = 0;
    if (!x || !out) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || W % 4 != 0 || (k != 5 && k != 7))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_shift_stack: needs W % 4 == 0 and k in {5, 7}");
    const int S = k == 5 ? 2 : 3;
    const long long work = (long long)N * S * S * C * (H + 2) * ((W + 4) / 4);
    const int blocks = grid_for(work, 16384);
    hipLaunchKernelGGL(thin::shift_stack, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), x, out, N, C, H, W, S, k);
    return check_launch("conv_shift_stack");
}

int tai_conv_cout1_3x3_forward(const float* x, const float* weight, const float* bias, float* y, int N, int Ci, int H,
                               int W, int act, void* hip_stream) {
    g_err[0] = 0;
    if (!x || !weight || !bias || !y) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || Ci <= 0 || H <= 0 || W <= 0 || W % 4 != 0 || act < 0 || act > 2)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv_cout1: needs W % 4 == 0, act in {0, 1, 2}");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const long long work = (long long)N * H * (W / 4);
    const int blocks = grid_for(work, 8192);
    auto kern = act == 0 ? thin::conv_cout1_3x3<0> : act == 1 ? thin::conv_cout1_3x3<1> : thin::conv_cout1_3x3<2>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, s, x, weight, bias, y, N, Ci, H, W);
    return check_launch("conv_cout1_3x3");
}

int tai_conv_cout1_5x5_forward(const float* x, const float* weight, const float* bias, float* y, int N, int Ci, int H, int W,
                               void* hip_stream) {
    g_err[0] = 0;
    if (!x || !weight || !y) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (N <= 0 || Ci <= 0 || H <= 0 || W <= 0 || W % 4 != 0) return fail(TAI_SEPCONV_EINVAL, "%s", "conv_cout1_5x5: needs W % 4 == 0");
    const long long work = (long long)N * H * (W / 4);
    const int blocks = grid_for(work, 8192);
    hipLaunchKernelGGL(thin::conv_cout1_5x5, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), x, weight, bias, y, N, Ci,
                       H, W);
    return check_launch("conv_cout1_5x5");
}

int tai_upsample_bilinear2x_backward(const float* grad_output, float* grad_input, int planes, int H, int W, void* hip_stream) {
    g_err[0] = 0;
    if (!grad_output || !grad_input) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (planes <= 0 || H <= 0 || W <= 0) return fail(TAI_SEPCONV_EINVAL, "%s", "bad dimensions");
    const float rh = (2 * H > 1) ? (float)(H - 1) / (float)(2 * H - 1) : 0.f;
    const float rw = (2 * W > 1) ? (float)(W - 1) / (float)(2 * W - 1) : 0.f;
    const long long work = (long long)planes * H * ((W + 3) / 4);
    const int blocks = grid_for(work, 65536);
    hipLaunchKernelGGL(ups::upsample2x_align_corners_backward, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
                       grad_output, grad_input, planes, H, W, rh, rw);
    return check_launch("upsample_bilinear2x_backward");
}

int tai_upsample_bilinear2x_forward(const float* input, float* output, int planes, int H, int W, void* hip_stream) {
    g_err[0] = 0;
    if (!input || !output) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (planes <= 0 || H <= 0 || W <= 0) return fail(TAI_SEPCONV_EINVAL, "%s", "bad dimensions");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    // ATen's area_pixel_compute_scale for align_corners = true, in fp32
    const float rh = (2 * H > 1) ? (float)(H - 1) / (float)(2 * H - 1) : 0.f;
    const float rw = (2 * W > 1) ? (float)(W - 1) / (float)(2 * W - 1) : 0.f;
    const long long total = (long long)planes * 2 * H * (2 * W);
    if ((2 * W) % 4 == 0 && H >= 2 && W >= 2 && (long long)H * W * 4 < (1LL << 30)) {
        // two output rows x four columns per thread from a 3 x 4 source window
        const int per_plane = H * (2 * W / 4);
        const int bx = grid_for(per_plane, 64);
        hipLaunchKernelGGL(ups::upsample2x_align_corners_pairs, dim3(bx, planes < 65535 ? planes : 65535), dim3(256), 0, s, input, output, planes, H, W,
                           rh, rw);
    } else if ((2 * W) % 4 == 0) {
        const long long threads = total / 4;
        const int blocks = grid_for(threads, 65536);
        hipLaunchKernelGGL(ups::upsample2x_align_corners_quads, dim3(blocks), dim3(256), 0, s, input, output, planes, H,
                           W, rh, rw);
    } else {
        const int blocks = grid_for(total, 65536);
        hipLaunchKernelGGL(ups::upsample2x_align_corners_scalar, dim3(blocks), dim3(256), 0, s, input, output, planes,
                           H, W, rh, rw);
    }
    return check_launch("upsample2x_align_corners");
}

}  // extern "C"
