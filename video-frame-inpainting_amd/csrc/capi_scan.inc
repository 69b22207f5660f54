// The frame scan (included by sepconv_capi.hip).

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

}  // extern "C"
