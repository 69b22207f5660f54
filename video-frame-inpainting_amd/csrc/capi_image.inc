// Image metrics, losses and the clip pipeline (included by sepconv_capi.hip).

// one workgroup per tile or chunk up to the kernel's GRID_CAP; past it a workgroup strides
static dim3 capped_grid(long long work, long long cap) { return dim3((unsigned)(work < cap ? work : cap)); }

// the pred[] / grad[] tables of imgloss::Args, temploss::Args and censusloss::Args: the caller's npred entries, null behind them and for every map
// when the caller passes no table
template <typename A>
static void fill_tables(A& a, const float* const* preds, float* const* grads, int npred) {
    for (int i = 0; i < (int)(sizeof(a.pred) / sizeof(a.pred[0])); ++i) {
        a.pred[i] = i < npred ? preds[i] : nullptr;
        a.grad[i] = (grads && i < npred) ? grads[i] : nullptr;
    }
}

extern "C" {

long long tai_frame_metrics_workspace_bytes(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H < 7 || W < 7) return TAI_SEPCONV_EINVAL;
    const fmetrics::Plan pl = fmetrics::plan(N, C, H, W);
    if (pl.tiles_total >= (1LL << 31)) return TAI_SEPCONV_EINVAL;
    return pl.tiles_total * (2 * (long long)sizeof(double) + (long long)sizeof(long long));
}

int tai_frame_metrics(const float* pred, const float* gt, long long* sse, double* ssim, double* l2, void* workspace, int N, int C,
                      int H, int W, void* hip_stream) {
    g_err[0] = 0;
    if (!pred || !gt || !sse || !ssim || !l2 || !workspace) return fail(TAI_SEPCONV_EINVAL, "%s", "frame_metrics: null pointer");
    if (N <= 0 || C <= 0 || H < 7 || W < 7)
        return fail(TAI_SEPCONV_EINVAL, "%s", "frame_metrics: needs N, C >= 1 and H, W >= 7 (the 7x7 SSIM window)");
    if ((long long)N * C * H * W >= (1LL << 40) || (long long)H * W >= (1LL << 31))
        return fail(TAI_SEPCONV_EINVAL, "%s", "frame_metrics: tensor too large");
    if (!aligned(workspace, 8)) return fail(TAI_SEPCONV_EINVAL, "%s", "frame_metrics: workspace must be 8-byte aligned");
    const fmetrics::Plan pl = fmetrics::plan(N, C, H, W);
    if (pl.tiles_total >= (1LL << 31)) return fail(TAI_SEPCONV_EINVAL, "%s", "frame_metrics: too many tiles (2^31 or more)");
    double* part_ssim = static_cast<double*>(workspace);
    double* part_l2 = part_ssim + pl.tiles_total;
    long long* part_sse = reinterpret_cast<long long*>(part_l2 + pl.tiles_total);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(fmetrics::tile_partials, dim3((unsigned)pl.tiles_total), dim3(fmetrics::THREADS), 0, s, pred, gt, part_ssim, part_l2,
                       part_sse, H, W, pl.nby, pl.nbx);
    if (int rc = check_launch("frame_metrics tile_partials")) return rc;
    hipLaunchKernelGGL(fmetrics::finish, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s, part_ssim, part_l2, part_sse, sse, ssim, l2, N, C, H,
                       W, pl.nby * pl.nbx);
    return check_launch("frame_metrics finish");
}

long long tai_ssim_loss_workspace_bytes(int N, int C, int H, int W) {
    if (ssimloss::refusal(N, C, H, W)) return TAI_SEPCONV_EINVAL;
    return ssimloss::plan(N, C, H, W).tiles_total * (long long)sizeof(double);
}

int tai_ssim_loss(const float* pred, const float* gt, double* plane_ssim, double* totals, float* grad, void* workspace, int N, int C,
                  int H, int W, void* hip_stream) {
    g_err[0] = 0;
    if (!pred || !gt || !plane_ssim || !totals || !workspace) return fail(TAI_SEPCONV_EINVAL, "%s", "ssim_loss: null pointer");
    if (const char* why = ssimloss::refusal(N, C, H, W, aligned(workspace, 8) && aligned(plane_ssim, 8) && aligned(totals, 8)))
        return fail(TAI_SEPCONV_EINVAL, "%s", why);
    const ssimloss::Plan pl = ssimloss::plan(N, C, H, W);
    const int planes = N * C;       // below 2^31: every plane has at least one tile
    double* part = static_cast<double*>(workspace);
    const double divisor = ((double)N * (double)C) * ((double)(H - 6) * (double)(W - 6));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(ssimloss::tile_loss_grad, dim3((unsigned)pl.tiles_total), dim3(ssimloss::THREADS), 0, s, pred, gt, part, grad, H, W,
                       pl.nby, pl.nbx, divisor);
    if (int rc = check_launch("ssim_loss tile_loss_grad")) return rc;
    hipLaunchKernelGGL(ssimloss::finish_planes, dim3((unsigned)((planes + ssimloss::THREADS - 1) / ssimloss::THREADS)), dim3(ssimloss::THREADS),
                       0, s, part, plane_ssim, planes, pl.nby * pl.nbx, H, W);
    if (int rc = check_launch("ssim_loss finish_planes")) return rc;
    hipLaunchKernelGGL(ssimloss::finish_total, dim3(1), dim3(ssimloss::THREADS), 0, s, plane_ssim, totals, planes);
    return check_launch("ssim_loss finish_total");
}

long long tai_image_loss_workspace_bytes(int npred, long long planes, int H, int W) {
    if (imgloss::refusal(npred, planes, H, W)) return TAI_SEPCONV_EINVAL;
    return npred * imgloss::plan(planes, H, W).tiles_total * 2 * (long long)sizeof(double);
}

int tai_image_loss(const float* const* preds, int npred, const float* gt, int kind, float eps, double* plane_terms, double* totals,
                   float* const* grads, void* workspace, long long planes, int H, int W, void* hip_stream) {
    g_err[0] = 0;
    if (!preds || !gt || !plane_terms || !totals || !workspace) return fail(TAI_SEPCONV_EINVAL, "%s", "image_loss: null pointer");
    if (const char* why = imgloss::refusal(npred, planes, H, W)) return fail(TAI_SEPCONV_EINVAL, "%s", why);
    if (kind < 0 || kind > 2) return fail(TAI_SEPCONV_EINVAL, "%s", "image_loss: kind must be 0 (L2), 1 (L1) or 2 (Charbonnier)");
    if (kind == 2 && !(std::isfinite(eps) && eps > 0.f))
        return fail(TAI_SEPCONV_EINVAL, "%s", "image_loss: the Charbonnier eps must be finite and > 0");
    for (int i = 0; i < npred; ++i)
        if (!preds[i]) return fail(TAI_SEPCONV_EINVAL, "%s", "image_loss: null prediction pointer");
    if (!aligned(workspace, 8) || !aligned(plane_terms, 8) || !aligned(totals, 8))
        return fail(TAI_SEPCONV_EINVAL, "%s", "image_loss: workspace, plane_terms and totals must be 8-byte aligned");
    const imgloss::Plan pl = imgloss::plan(planes, H, W);
    imgloss::Args a;
    fill_tables(a, preds, grads, npred);
    a.gt = gt;
    a.part = static_cast<double*>(workspace);
    a.npred = npred; a.kind = kind; a.H = H; a.W = W; a.nby = pl.nby; a.nbx = pl.nbx;
    a.tiles_total = pl.tiles_total;
    a.e2 = kind == 2 ? eps * eps : 0.f;
    a.cp = 0.5 / (((double)planes * (double)H) * (double)W);
    a.cg = 0.5 / (((double)planes * (double)(H - 1)) * (double)(W - 1));
    const long long rows = npred * planes;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(imgloss::tile_loss_grad, capped_grid(pl.tiles_total, imgloss::GRID_CAP), dim3(imgloss::THREADS), 0, s, a);
    if (int rc = check_launch("image_loss tile_loss_grad")) return rc;
    hipLaunchKernelGGL(imgloss::finish_planes, dim3((unsigned)((rows + imgloss::THREADS - 1) / imgloss::THREADS)), dim3(imgloss::THREADS), 0, s,
                       a.part, plane_terms, rows, pl.nby * pl.nbx);
    if (int rc = check_launch("image_loss finish_planes")) return rc;
    hipLaunchKernelGGL(imgloss::finish_total, dim3((unsigned)npred), dim3(imgloss::THREADS), 0, s, plane_terms, totals, planes,
                       ((double)planes * (double)H) * (double)W, ((double)planes * (double)(H - 1)) * (double)(W - 1));
    return check_launch("image_loss finish_total");
}

long long tai_lap_loss_workspace_bytes(long long planes, int H, int W, int levels) {
    if (laploss::refusal(planes, H, W, levels)) return TAI_SEPCONV_EINVAL;
    return laploss::plan(planes, H, W, levels).work_bytes;
}

int tai_lap_loss(const float* pred, const float* gt, int levels, double* plane_terms, double* totals, float* grad, void* workspace,
                 long long planes, int H, int W, void* hip_stream) {
    g_err[0] = 0;
    if (!pred || !gt || !plane_terms || !totals || !workspace) return fail(TAI_SEPCONV_EINVAL, "%s", "lap_loss: null pointer");
    if (const char* why = laploss::refusal(planes, H, W, levels)) return fail(TAI_SEPCONV_EINVAL, "%s", why);
    if (!aligned(workspace, 8) || !aligned(plane_terms, 8) || !aligned(totals, 8))
        return fail(TAI_SEPCONV_EINVAL, "%s", "lap_loss: workspace, plane_terms and totals must be 8-byte aligned");
    laploss::Plan pl = laploss::plan(planes, H, W, levels);
    pl.a.pred = pred;
    pl.a.gt = gt;
    pl.a.grad = grad;
    pl.a.plane_terms = plane_terms;
    pl.a.work = static_cast<double*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(pl.in_lds ? laploss::pyramid_lds : laploss::pyramid_workspace, dim3(pl.grid), dim3(laploss::THREADS), 0, s, pl.a);
    if (int rc = check_launch("lap_loss pyramid")) return rc;
    hipLaunchKernelGGL(laploss::finish_total, dim3(1), dim3(laploss::FIN_THREADS), 0, s, plane_terms, totals, planes, levels, pl.a.count);
    return check_launch("lap_loss finish_total");
}

long long tai_temporal_loss_workspace_bytes(int npred, int B, int T, int C, int H, int W) {
    if (temploss::refusal(npred, B, T, C, H, W)) return TAI_SEPCONV_EINVAL;
    return npred * temploss::plan((long long)B * C, H, W).chunks_total * ((long long)T + 1) * temploss::WAVES * (long long)sizeof(double);
}

int tai_temporal_loss(const float* const* preds, int npred, const float* gt, const long long* strides, int kind, float eps,
                      double* seq_terms, double* totals, float* const* grads, void* workspace, int B, int T, int C, int H, int W,
                      void* stream) {
    g_err[0] = 0;
    if (const char* why = temploss::call_refusal(preds, npred, gt, strides, kind, eps, seq_terms, totals, workspace, B, T, C, H, W))
        return fail(TAI_SEPCONV_EINVAL, "%s", why);
    const long long S = (long long)B * C;
    const temploss::Plan pl = temploss::plan(S, H, W);
    temploss::Args a;
    fill_tables(a, preds, grads, npred);
    for (int i = 0; i < temploss::MAXP; ++i) {
        a.sb[i] = i < npred ? strides[2 * i] : 0;
        a.st[i] = i < npred ? strides[2 * i + 1] : 0;
    }
    a.gt = gt;
    a.sb[temploss::MAXP] = strides[2 * npred];
    a.st[temploss::MAXP] = strides[2 * npred + 1];
    a.part = static_cast<double*>(workspace);
    a.npred = npred; a.kind = kind; a.T = T; a.C = C; a.H = H; a.W = W;
    a.rpr = pl.rpr; a.cps = pl.cps; a.runs = pl.runs; a.chunks_total = pl.chunks_total;
    a.e2 = kind == 2 ? eps * eps : 0.f;
    const double n_pos = ((double)S * (double)H) * (double)W;                 // integers below 2^41: exact
    const double count = n_pos * (double)(T + 1);
    a.ct = 0.5 / count;
    const long long rows = npred * S * (T + 1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(temploss::walk_loss_grad, capped_grid(pl.chunks_total, temploss::GRID_CAP), dim3(temploss::THREADS), 0, s, a);
    if (int rc = check_launch("temporal_loss walk_loss_grad")) return rc;
    hipLaunchKernelGGL(temploss::finish_sequences, dim3((unsigned)((rows + temploss::THREADS - 1) / temploss::THREADS)), dim3(temploss::THREADS),
                       0, s, a.part, seq_terms, rows, S, T + 1, pl.cps);
    if (int rc = check_launch("temporal_loss finish_sequences")) return rc;
    hipLaunchKernelGGL(temploss::finish_total, dim3((unsigned)npred), dim3(temploss::THREADS), 0, s, seq_terms, totals, S, T + 1, n_pos, count);
    return check_launch("temporal_loss finish_total");
}

long long tai_census_loss_workspace_bytes(int npred, int B, int T, int C, int H, int W) {
    if (censusloss::refusal(npred, B, T, C, H, W)) return TAI_SEPCONV_EINVAL;
    return npred * censusloss::plan(B, T, H, W).tiles_total * (long long)sizeof(double);
}

int tai_census_loss(const float* const* preds, int npred, const float* gt, const long long* strides, double* frame_terms, double* totals,
                    float* const* grads, void* workspace, int B, int T, int C, int H, int W, void* stream) {
    g_err[0] = 0;
    if (const char* why = censusloss::call_refusal(preds, npred, gt, strides, frame_terms, totals, workspace, B, T, C, H, W))
        return fail(TAI_SEPCONV_EINVAL, "%s", why);
    const censusloss::Plan pl = censusloss::plan(B, T, H, W);
    censusloss::Args a;
    fill_tables(a, preds, grads, npred);
    for (int i = 0; i < censusloss::MAXP; ++i) {
        a.sb[i] = i < npred ? strides[2 * i] : 0;
        a.st[i] = i < npred ? strides[2 * i + 1] : 0;
    }
    a.gt = gt;
    a.sb[censusloss::MAXP] = strides[2 * npred];
    a.st[censusloss::MAXP] = strides[2 * npred + 1];
    a.part = static_cast<double*>(workspace);
    a.npred = npred; a.T = T; a.C = C; a.H = H; a.W = W; a.nby = pl.nby; a.nbx = pl.nbx;
    a.tiles_total = pl.tiles_total;
    const double interior = (double)(H - 6) * (double)(W - 6);                 // integers below 2^31 and 2^62 / 2^11: exact
    const double count = (double)pl.frames * interior;
    a.kappa = (255.0 * 0.5) / (49.0 * count);
    const long long rows = npred * pl.frames;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(C == 1 ? censusloss::tile_loss_grad<1> : censusloss::tile_loss_grad<3>, capped_grid(pl.tiles_total, censusloss::GRID_CAP),
                       dim3(censusloss::THREADS), 0, s, a);
    if (int rc = check_launch("census_loss tile_loss_grad")) return rc;
    hipLaunchKernelGGL(censusloss::finish_frames, dim3((unsigned)((rows + censusloss::THREADS - 1) / censusloss::THREADS)),
                       dim3(censusloss::THREADS), 0, s, a.part, frame_terms, rows, pl.nby * pl.nbx, interior);
    if (int rc = check_launch("census_loss finish_frames")) return rc;
    hipLaunchKernelGGL(censusloss::finish_total, dim3((unsigned)npred), dim3(censusloss::THREADS), 0, s, frame_terms, totals, pl.frames);
    return check_launch("census_loss finish_total");
}

int tai_clip_from_frames(const unsigned char* frames, long long frames_bytes, const long long* table, const long long* table_host,
                         const float* levels, float* out, int N, int c_dim, int H, int W, int pad_h, int pad_w, void* hip_stream) {
    g_err[0] = 0;
    if (!frames || !table || !table_host || !levels || !out) return fail(TAI_SEPCONV_EINVAL, "%s", "clip_from_frames: null pointer");
    if (c_dim != 1 && c_dim != 3) return fail(TAI_SEPCONV_EINVAL, "%s", "clip_from_frames: c_dim must be 1 or 3");
    if (N <= 0 || H <= 0 || W <= 0 || pad_h < 0 || pad_w < 0 || frames_bytes <= 0)
        return fail(TAI_SEPCONV_EINVAL, "%s", "clip_from_frames: needs N, H, W, frames_bytes > 0 and pad_h, pad_w >= 0");
    const long long Hp = (long long)H + pad_h, Wp = (long long)W + pad_w;
    if (Hp >= (1LL << 24) || Wp >= (1LL << 24) || (long long)N * c_dim * Hp * Wp >= (1LL << 31) || frames_bytes >= (1LL << 40))
        return fail(TAI_SEPCONV_EINVAL, "%s", "clip_from_frames: index space too large (2^31 output elements or more)");
    for (int n = 0; n < N; ++n) {
        const long long off = table_host[4 * n], h = table_host[4 * n + 1], w = table_host[4 * n + 2];
        if (h <= 0 || w <= 0 || h >= (1LL << 24) || w >= (1LL << 24))
            return fail(TAI_SEPCONV_EINVAL, "%s", "clip_from_frames: a frame descriptor has a non-positive or oversized source size");
        if (off < 0 || off > frames_bytes || h * w * 3 > frames_bytes - off)
            return fail(TAI_SEPCONV_EINVAL, "%s", "clip_from_frames: a frame descriptor points past the stated length of the frame buffer");
    }
    const bool vec4 = Wp % 4 == 0 && aligned(out, 16);
    const int runs_per_row = (int)((Wp + 3) / 4);
    const long long total_runs = (long long)N * Hp * runs_per_row;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const dim3 grid(clip::blocks_for(total_runs)), block(clip::THREADS);
    auto kern = c_dim == 1 ? (vec4 ? clip::from_frames<1, true> : clip::from_frames<1, false>) : (vec4 ? clip::from_frames<3, true> : clip::from_frames<3, false>);
    hipLaunchKernelGGL(kern, grid, block, 0, s, frames, frames_bytes, table, levels, out, N, H, W, (int)Hp, (int)Wp, runs_per_row, total_runs);
    return check_launch("clip_from_frames");
}

int tai_clip_from_frames_aug(const unsigned char* frames, long long frames_bytes, const long long* table, const long long* table_host,
                             const float* tables, int n_tables, const float* levels, float* out, int N, int c_dim, int H, int W, int pad_h,
                             int pad_w, void* stream) {
    g_err[0] = 0;
    if (const char* why = clipaug::call_refusal(frames, frames_bytes, table, table_host, tables, n_tables, levels, out, N, c_dim, H, W, pad_h, pad_w))
        return fail(TAI_SEPCONV_EINVAL, "%s", why);
    const long long Hp = (long long)H + pad_h, Wp = (long long)W + pad_w;
    const clipaug::Geometry g = clipaug::geometry(Hp, Wp);
    const long long items = (long long)N * g.bands;
    const bool vec4 = Wp % 4 == 0 && aligned(out, 16);
    auto kern = c_dim == 1 ? (vec4 ? clipaug::from_frames_aug<1, true> : clipaug::from_frames_aug<1, false>)
                           : (vec4 ? clipaug::from_frames_aug<3, true> : clipaug::from_frames_aug<3, false>);
    hipLaunchKernelGGL(kern, capped_grid(items, clipaug::GRID_CAP), dim3(clipaug::THREADS), 0, static_cast<hipStream_t>(stream), frames,
                       frames_bytes, table, tables, n_tables, levels, out, H, W, (int)Hp, (int)Wp, g.runs_per_row, g.rw, g.band_rows, g.bands,
                       items);
    return check_launch("clip_from_frames_aug");
}

int tai_frames_to_uint8(const float* x, unsigned char* out, int N, int C, int Hs, int Ws, int h, int w, int reverse_channels,
                        void* hip_stream) {
    g_err[0] = 0;
    if (!x || !out) return fail(TAI_SEPCONV_EINVAL, "%s", "frames_to_uint8: null pointer");
    if (C != 1 && C != 3) return fail(TAI_SEPCONV_EINVAL, "%s", "frames_to_uint8: C must be 1 or 3");
    if (N <= 0 || Hs <= 0 || Ws <= 0 || h <= 0 || w <= 0 || h > Hs || w > Ws)
        return fail(TAI_SEPCONV_EINVAL, "%s", "frames_to_uint8: needs N > 0 and 0 < h <= Hs, 0 < w <= Ws");
    if ((long long)N * C * Hs * Ws >= (1LL << 31)) return fail(TAI_SEPCONV_EINVAL, "%s", "frames_to_uint8: index space too large (2^31 elements or more)");
    const long long total = (long long)N * h * w;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const dim3 grid(clip::blocks_for(total)), block(clip::THREADS);
    hipLaunchKernelGGL(C == 1 ? clip::to_uint8<1> : clip::to_uint8<3>, grid, block, 0, s, x, out, Hs, Ws, h, w, reverse_channels != 0, total);
    return check_launch("frames_to_uint8");
}

}  // extern "C"
