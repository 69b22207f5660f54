// The frame scan, the block scan and the composite of partly damaged frames (included by sepconv_capi.hip).

extern "C" {

long long tai_frame_scan_workspace_bytes(long long n_frames, long long frame_bytes) {
    if (fscan::refusal(n_frames, frame_bytes)) return TAI_SEPCONV_EINVAL;
    return n_frames * fscan::max_segments(frame_bytes) * fscan::STATS * (long long)sizeof(long long);
}

int tai_frame_scan(const unsigned char* frames, long long n_frames, long long frame_bytes, int tol, long long* stats, void* workspace,
                   void* stream) {
    g_err[0] = 0;
    if (const char* why = fscan::call_refusal(frames, n_frames, frame_bytes, tol, stats, workspace)) return fail(TAI_SEPCONV_EINVAL, "%s", why);
    fscan::Args a = fscan::plan(n_frames, frame_bytes, (int)(reinterpret_cast<uintptr_t>(frames) % fscan::VEC_BYTES));
    a.frames = frames;
    a.part = static_cast<long long*>(workspace);
    a.tol = tol;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool vec = frame_bytes % fscan::VEC_BYTES == 0;
    auto kern = vec ? (tol == 0 ? fscan::walk<true, true> : fscan::walk<true, false>) : (tol == 0 ? fscan::walk<false, true> : fscan::walk<false, false>);
    hipLaunchKernelGGL(kern, capped_grid(a.items, fscan::GRID_CAP), dim3(fscan::THREADS), 0, s, a);
    if (int rc = check_launch("frame_scan walk")) return rc;
    const long long waves = fscan::THREADS / 64;
    hipLaunchKernelGGL(fscan::finish, capped_grid((n_frames + waves - 1) / waves, fscan::GRID_CAP), dim3(fscan::THREADS), 0, s, a.part, stats,
                       n_frames, a.nseg);
    return check_launch("frame_scan finish");
}

long long tai_block_scan_workspace_bytes(long long n_frames, int h, int w, int c, int bs) {
    if (bscan::refusal(n_frames, h, w, c, bs)) return TAI_SEPCONV_EINVAL;
    return bscan::workspace_bytes(n_frames, h, w, c, bs);
}

int tai_block_scan(const unsigned char* frames, long long n_frames, int h, int w, int c, int bs, int tol, long long* stats, void* workspace,
                   void* stream) {
    g_err[0] = 0;
    if (const char* why = bscan::call_refusal(frames, n_frames, h, w, c, bs, tol, stats, workspace)) return fail(TAI_SEPCONV_EINVAL, "%s", why);
    bscan::Args a = bscan::plan(n_frames, h, w, c, bs);
    a.frames = frames;
    a.stats = stats;
    a.tol = tol;
    hipLaunchKernelGGL(tol == 0 ? bscan::walk<true> : bscan::walk<false>, capped_grid(a.items, bscan::GRID_CAP), dim3(bscan::THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    return check_launch("block_scan");
}

int tai_damage_composite(const float* pred, long long pred_elems, const float* src, long long src_elems, const long long* table,
                         const long long* table_host, long long n_items, const unsigned char* blocks, long long n_maps, int Bh, int Bw,
                         int bs, const int* r0, const int* r1, const int* c0, const int* c1, unsigned char* out, long long n_out, int C,
                         int Hs, int Ws, int h, int w, int feather, int reverse_channels, void* stream) {
    g_err[0] = 0;
    if (const char* why = dcomp::refusal(pred, pred_elems, src, src_elems, table, table_host, n_items, blocks, n_maps, Bh, Bw, bs, r0, r1, c0,
                                         c1, out, n_out, C, Hs, Ws, h, w, feather))
        return fail(TAI_SEPCONV_EINVAL, "%s", why);
    dcomp::Args a = {};
    a.pred = pred; a.src = src; a.pred_elems = pred_elems; a.src_elems = src_elems;
    a.table = table; a.n_items = n_items; a.n_maps = n_maps; a.n_out = n_out;
    a.blocks = blocks; a.r0 = r0; a.r1 = r1; a.c0 = c0; a.c1 = c1; a.out = out;
    a.Bh = Bh; a.Bw = Bw; a.bs = bs; a.Hs = Hs; a.Ws = Ws; a.h = h; a.w = w; a.feather = feather; a.reverse = reverse_channels != 0;
    a.tiles_y = (h + dcomp::TILE_H - 1) / dcomp::TILE_H;
    a.tiles_x = (w + dcomp::TILE_W - 1) / dcomp::TILE_W;
    a.work = n_items * a.tiles_y * a.tiles_x;
    const bool vec = (long long)w * C % 16 == 0 && aligned(out, 16);      // then every row of every output frame is 16-byte aligned
    auto kern = C == 1 ? (vec ? dcomp::composite<1, true> : dcomp::composite<1, false>) : (vec ? dcomp::composite<3, true> : dcomp::composite<3, false>);
    hipLaunchKernelGGL(kern, capped_grid(a.work, dcomp::GRID_CAP), dim3(dcomp::THREADS), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("damage_composite");
}

}  // extern "C"
