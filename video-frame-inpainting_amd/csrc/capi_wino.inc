// Winograd F(2x2, 3x3) entry points (included by sepconv_capi.hip).

namespace {

// the instance of wino::conv3x3<ACT, DBG, SKIP, PARTS, TALL, EPI> for the workgroup shape, and for the activation
using WinoKernel = decltype(&wino::conv3x3<0>);
template <int A, int D, int SK, int Q, int E>
WinoKernel wino_kernel(bool tall) { return tall ? wino::conv3x3<A, D, SK, Q, true, E> : wino::conv3x3<A, D, SK, Q, false, E>; }
template <int Q, int E>
WinoKernel wino_kernel_act(int act, bool tall) {
    return act == 0 ? wino_kernel<0, 0, 0, Q, E>(tall) : act == 1 ? wino_kernel<1, 0, 0, Q, E>(tall) : wino_kernel<2, 0, 0, Q, E>(tall);
}

// the instance of wino::split::conv3x3<ACT, PARTS, EPI, EDGE> for cat operands and planes that need the edge handling
template <int A, int E>
decltype(&wino::split::conv3x3<0, 0, 0, false>) wino_split_kernel(bool parts, bool edge) {
    return parts ? (edge ? wino::split::conv3x3<A, 1, E, true> : wino::split::conv3x3<A, 1, E, false>)
                 : (edge ? wino::split::conv3x3<A, 0, E, true> : wino::split::conv3x3<A, 0, E, false>);
}

}  // namespace

extern "C" {

// Arithmetic of the Winograd GEMMs: 0 = fp32 MFMA (the default; every parity claim), 1 = split bf16 (three terms, six products,
// fp32 accumulation: wino_split.hip.inc), opt-in.  The mode decides what tai_conv3x3_wino_weight_floats / _transform_weights
// produce: in mode 1 the buffer holds the fp32 image FOLLOWED by the split image, and the buffer is remembered, so that the forward
// entry points follow the BUFFER they are handed (a shape the split kernel does not take runs the fp32 kernel on the same buffer)
// and a buffer made in one mode can never be read in the other's layout.
static std::atomic<int> g_wino_arith{0};
static std::mutex g_split_mu;
static std::unordered_set<const void*> g_split_bufs;
int tai_conv3x3_wino_set_arithmetic(int mode) {
    g_err[0] = 0;
    if (mode != 0 && mode != 1) return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_set_arithmetic: 0 (fp32 MFMA) or 1 (split bf16)");
    return g_wino_arith.exchange(mode, std::memory_order_relaxed);
}
int tai_conv3x3_wino_get_arithmetic(void) { return g_wino_arith.load(std::memory_order_relaxed); }
// the caller is about to free (or has freed) a buffer that tai_conv3x3_wino_transform_weights wrote: drop its layout record
int tai_conv3x3_wino_forget_weights(const float* U) {
    std::lock_guard<std::mutex> lk(g_split_mu);
    return (int)g_split_bufs.erase(U);
}

long long tai_conv3x3_wino_weight_floats(int K, int C) {
    if (K <= 0 || C <= 0) return 0;
    const long long Kpad = (K + wino::TM - 1) / wino::TM * wino::TM, Cpad = (C + wino::KC - 1) / wino::KC * wino::KC;
    // (split image: 16 positions x 3 bf16 terms per weight = 24 floats' worth)
    return (g_wino_arith.load(std::memory_order_relaxed) == 1 ? 40 : 16) * Kpad * Cpad;
}

int tai_conv3x3_wino_transform_weights(const float* weight, float* U, int K, int C, void* hip_stream) {
    g_err[0] = 0;
    if (!weight || !U || K <= 0 || C <= 0) return fail(TAI_SEPCONV_EINVAL, "%s", "wino transform_weights: bad argument");
    const int Kpad = (K + wino::TM - 1) / wino::TM * wino::TM, Cpad = (C + wino::KC - 1) / wino::KC * wino::KC;
    const long long total = (long long)Kpad * Cpad;
    const int blocks = grid_for(total, 4096);
    const bool split = g_wino_arith.load(std::memory_order_relaxed) == 1;
    {
        std::lock_guard<std::mutex> lk(g_split_mu);
        if (split) g_split_bufs.insert(U); else g_split_bufs.erase(U);
    }
    hipLaunchKernelGGL(wino::transform_weights, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), weight, U, K,
                       C, Kpad, Cpad);
    if (split)
        hipLaunchKernelGGL(wino::split::transform_weights, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), weight,
                           reinterpret_cast<unsigned short*>(U + 16 * total), K, C, Kpad, Cpad);
    return check_launch("wino_transform_weights");
}

// Split of the weight-gradient kernel's reduction (the tiles) over workgroups: about one workgroup per CU in total.
// ragged: any other H and W than even H with W % 16 == 0 -- the kernel's variant over the planes zero-extended to an even number
// of rows and roundup(W, 16) columns (wino::wrw::WRW_RAGGED); the shapes the kernel took before keep their plan.
struct WrwPlan { int kblocks, cblocks, nchunks, chunks_per_split, splits, pair, ragged; };
static bool wrw_plan(int N, int C, int K, int H, int W, WrwPlan& p, int in_h = 0, int in_w = 0) {
    if (N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0) return false;
    if (in_h <= 0) { in_h = H; in_w = W; }
    if ((long long)N * C * in_h * in_w * 4 >= (1LL << 31) || (long long)N * K * H * W * 4 >= (1LL << 31)) return false;
    p.ragged = H % 2 != 0 || W % 16 != 0;
    const int Hx = (H + 1) / 2 * 2, Wx = (W + 15) / 16 * 16;          // the extended planes (H, W unless ragged)
    if ((long long)N * (Hx / 2) * (Wx / 2) / wino::wrw::CT >= (1LL << 31)) return false;
    p.kblocks = (K + 63) / 64;
    p.cblocks = (C + 63) / 64;
    p.nchunks = (int)((long long)N * (Hx / 2) * (Wx / 2) / wino::wrw::CT);
    int want = 256 / (p.kblocks * p.cblocks);
    if (want < 1) want = 1;
    if (want > p.nchunks) want = p.nchunks;
    p.chunks_per_split = (p.nchunks + want - 1) / want;
    p.pair = !p.ragged && W % 32 == 0;            // chunk pairs over 16 consecutive tiles: whole 128-byte lines per load
    if (p.pair && (p.chunks_per_split & 1)) ++p.chunks_per_split;      // (the chunk count is even when W % 32 == 0)
    p.splits = (p.nchunks + p.chunks_per_split - 1) / p.chunks_per_split;
    return true;
}

// The same gradient in the F(4x4, 3x3) domain (wino43::conv3x3_wrw_gen): blocks of 64 output x 32 input channels, chunks of four tiles
// (16 pixels of a row), the run of chunks split over about one workgroup per CU; the slabs have the F(2x2) kernel's layout
// [split][tap][Kpad][Cpad] (Cpad a multiple of 64) and go through the same wrw_reduce.
static bool wrw43_plan(int N, int C, int K, int H, int W, WrwPlan& p, int in_h = 0, int in_w = 0, int in_oy = 0, int in_ox = 0) {
    if (N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0 || H % 4 != 0 || W % 16 != 0) return false;
    if (in_h <= 0) { in_h = H; in_w = W; }
    // an input plane with a halo must hold the whole one-pixel frame of the output window (nothing is padded then)
    if ((in_h != H || in_w != W) && (in_oy < 1 || in_ox < 1 || in_oy + H + 1 > in_h || in_ox + W + 1 > in_w)) return false;
    if ((long long)N * C * in_h * in_w * 4 + (in_w + 1) * 4 >= (1LL << 31) || (long long)N * K * H * W * 4 >= (1LL << 31)) return false;
    p.kblocks = (K + 63) / 64;
    p.cblocks = (C + 31) / 32;
    p.nchunks = (int)((long long)N * (H / 4) * (W / 16));
    // splits: one workgroup per CU where the blocks divide the 256 CUs; otherwise the count (up to 32, at least 16 chunks each) whose
    // last round of workgroups is fullest -- 144 blocks (the 7x7 layer's stack: 36 x 4) as 1 split leave 112 CUs idle for the whole
    // kernel, as 7 splits 4 rounds of 252 run in 0.57 of that time
    const int blocks = p.kblocks * p.cblocks;
    int want = 1;
    double best = 1e30;
    auto rounds_per_split = [&](int sp) { return (double)((blocks * sp + 255) / 256) / sp; };
    for (int sp = 1; sp <= 32 && sp <= p.nchunks && (sp == 1 || p.nchunks / sp >= 16); ++sp) best = rounds_per_split(sp) < best ? rounds_per_split(sp) : best;
    for (int sp = 1; sp <= 32; ++sp)                 // the smallest count within 3 % of the best (every split writes a slab and runs an epilogue)
        if (rounds_per_split(sp) <= 1.03 * best) { want = sp; break; }
    if (blocks * want < 256) {                       // fewer workgroups than CUs in one round: as many splits as fill it
        want = 256 / blocks;
        if (want > p.nchunks) want = p.nchunks;
    }
    p.chunks_per_split = (p.nchunks + want - 1) / want;
    p.splits = (p.nchunks + p.chunks_per_split - 1) / p.chunks_per_split;
    p.pair = 0;
    return true;
}

static std::atomic<int> g_wrw_tile{4};              // 4 (default): the F(4x4, 3x3)-domain kernel where its shape rules allow, 2: F(2x2, 3x3) always
int tai_conv3x3_wino_wrw_set_tile(int tile) {
    if (tile != 2 && tile != 4) return -1;
    return g_wrw_tile.exchange(tile, std::memory_order_relaxed);
}

long long tai_conv3x3_wino_wrw_workspace_floats(int N, int C, int K, int H, int W) {
    WrwPlan p, q;
    if (!wrw_plan(N, C, K, H, W, p)) return -1;
    long long need = (long long)p.splits * 9 * p.kblocks * 64 * p.cblocks * 64 + (long long)p.splits * p.kblocks * 64;     // taps, then bias partials
    if (wrw43_plan(N, C, K, H, W, q)) {              // (either kernel may serve the call: tai_conv3x3_wino_wrw_set_tile)
        const long long n43 = (long long)q.splits * 9 * q.kblocks * 64 * ((C + 63) / 64 * 64) + (long long)q.splits * q.kblocks * 64;
        if (n43 > need) need = n43;
    }
    return need;
}

static std::atomic<int> g_wrw_pair{1};              // 1: paired chunks (whole-line loads) when W % 32 == 0
int tai_conv3x3_wino_wrw_set_paired(int on) { return g_wrw_pair.exchange(on ? 1 : 0, std::memory_order_relaxed); }

// THE decision of a weight-gradient launch (wino_wrw_impl below, and through it every entry point, and tai_conv3x3_wino_wrw_plan): the
// refusals that depend on the dimensions alone, then the transform domain (tile 4: wino43::conv3x3_wrw_gen where its shape rules allow
// and tai_conv3x3_wino_wrw_set_tile has not chosen 2) with that kernel's plan, and the load scheme of the F(2x2) kernel.  Returns 0, or
// the refusal (fail).  in_h <= 0: no window (the plane is H x W at (0, 0)).
struct WrwRoute { int tile, pair; WrwPlan p; };
static int wrw_route(int N, int C, int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, bool stamps, WrwRoute& r) {
    if (in_h <= 0) { in_h = H; in_w = W; in_oy = in_ox = 0; }
    else if (in_w <= 0) return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_wrw_window: bad plane");      // (the window launcher's own words)
    // the window of every tile must lie inside the plane or in its zero padding on all sides consistently: the origin may
    // not be negative and an input with a halo (origin > 0) must hold the whole 1-pixel frame
    if (in_oy < 0 || in_ox < 0 || in_oy + H > in_h || in_ox + W > in_w)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_wrw: output window outside the input plane");
    if (!wrw_plan(N, C, K, H, W, r.p, in_h, in_w))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_wrw: needs positive dimensions and tensors below 2 GiB");
    if (r.p.ragged && stamps)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_wrw: timeline stamps need even H and W % 16 == 0");
    WrwPlan q;
    if (g_wrw_tile.load(std::memory_order_relaxed) == 4 && !stamps && wrw43_plan(N, C, K, H, W, q, in_h, in_w, in_oy, in_ox)) {
        r.tile = 4;
        r.pair = 0;
        r.p = q;
        r.p.ragged = 0;
        return 0;
    }
    r.tile = 2;
    r.pair = r.p.pair && g_wrw_pair.load(std::memory_order_relaxed) ? 1 : 0;
    return 0;
}

// The route of a launch as a query: the same wrw_route call, hence the same refusals with the same words, as tai_conv3x3_wino_wrw
// (in_h <= 0) / tai_conv3x3_wino_wrw_window make for these dimensions.  No stream, no launch.
int tai_conv3x3_wino_wrw_plan(int N, int C, int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, int* out) {
    g_err[0] = 0;
    if (!out) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    WrwRoute r;
    if (int rc = wrw_route(N, C, K, H, W, in_h, in_w, in_oy, in_ox, false, r)) return rc;
    const int v[8] = {r.tile, r.pair, r.p.ragged, r.p.kblocks, r.p.cblocks, r.p.nchunks, r.p.chunks_per_split, r.p.splits};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return r.p.kblocks * r.p.cblocks * r.p.splits;
}

static int wino_wrw_impl(const float* x, const float* dy, float* dw, float* dbias, float* workspace, int N, int C, int K, int H,
                         int W, void* hip_stream, long long* stamps, int in_h = 0, int in_w = 0, int in_oy = 0, int in_ox = 0) {
    g_err[0] = 0;
    if (!x || !dy || !dw || !workspace) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (in_h <= 0) { in_h = H; in_w = W; in_oy = in_ox = 0; }
    WrwRoute r;
    if (int rc = wrw_route(N, C, K, H, W, in_h, in_w, in_oy, in_ox, stamps != nullptr, r)) return rc;
    const WrwPlan& p = r.p;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (r.tile == 4) {
        const WrwPlan& q = r.p;
        const int Kpad = q.kblocks * 64, Cpad = (C + 63) / 64 * 64;
        float* wsb43 = dbias ? workspace + (long long)q.splits * 9 * Kpad * Cpad : nullptr;
        if (int rc = launch(wino43::conv3x3_wrw_gen, dim3((unsigned)(q.kblocks * q.cblocks * q.splits)), dim3(512), wino43::WRW_LDS_BYTES, stream, x, dy,
                            workspace, wsb43, N, C, K, H, W, q.kblocks, q.cblocks, Kpad, Cpad, q.chunks_per_split, q.nchunks, in_h, in_w, in_oy, in_ox,
                            g_wino43_placement.load(std::memory_order_relaxed) ? 0 : 1))
            return rc;
        if (int rc = check_launch("conv3x3_wino43_wrw")) return rc;
        const long long rows43 = 9LL * K * (Cpad / 64);
        const int blocks43 = (int)(rows43 < 8192 ? (rows43 < q.kblocks ? q.kblocks : rows43) : 8192);
        hipLaunchKernelGGL(wino::wrw::wrw_reduce, dim3(blocks43), dim3(256), 0, stream, workspace, dw, wsb43, dbias, K, C, Kpad, Cpad, q.splits);
        return check_launch("conv3x3_wino43_wrw_reduce");
    }
    const int grid = p.kblocks * p.cblocks * p.splits;
    float* wsb = dbias ? workspace + (long long)p.splits * 9 * p.kblocks * 64 * p.cblocks * 64 : nullptr;
    const bool pair = r.pair != 0;
    auto kern = pair ? wino::wrw::conv3x3_wrw<0, true> : wino::wrw::conv3x3_wrw<0, false>;
    if (stamps) kern = pair ? wino::wrw::conv3x3_wrw<2, true> : wino::wrw::conv3x3_wrw<2, false>;
    else if (p.ragged) kern = wino::wrw::conv3x3_wrw<wino::wrw::WRW_RAGGED, false>;
    if (int rc = launch(kern, dim3(grid), dim3(256), wino::wrw::LDS_BYTES, stream, x, dy, workspace, wsb, N, C, K, H, W, in_h, in_w, in_oy, in_ox,
                        p.kblocks, p.cblocks, p.chunks_per_split, p.nchunks, stamps))
        return rc;
    if (int rc = check_launch("conv3x3_wino_wrw")) return rc;
    const long long rows = 9LL * K * p.cblocks;
    const int blocks = (int)(rows < 8192 ? (rows < p.kblocks ? p.kblocks : rows) : 8192);      // (at least one workgroup per 64 bias entries)
    hipLaunchKernelGGL(wino::wrw::wrw_reduce, dim3(blocks), dim3(256), 0, stream, workspace, dw, wsb, dbias, K, C,
                       p.kblocks * 64, p.cblocks * 64, p.splits);
    return check_launch("conv3x3_wino_wrw_reduce");
}

int tai_conv3x3_wino_wrw(const float* x, const float* dy, float* dw, float* dbias, float* workspace, int N, int C, int K, int H,
                         int W, void* hip_stream) {
    return wino_wrw_impl(x, dy, dw, dbias, workspace, N, C, K, H, W, hip_stream, nullptr);
}

int tai_conv3x3_wino_wrw_window(const float* x, const float* dy, float* dw, float* dbias, float* workspace, int N, int C, int K,
                                int H, int W, int in_h, int in_w, int in_oy, int in_ox, void* hip_stream) {
    if (in_h <= 0 || in_w <= 0) { g_err[0] = 0; return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_wrw_window: bad plane"); }
    return wino_wrw_impl(x, dy, dw, dbias, workspace, N, C, K, H, W, hip_stream, nullptr, in_h, in_w, in_oy, in_ox);
}

#ifdef TAI_TIMING_VARIANTS
int tai_conv3x3_wino_wrw_timeline(const float* x, const float* dy, float* dw, float* workspace, int N, int C, int K, int H,
                                  int W, long long* stamps, void* hip_stream) {
    return wino_wrw_impl(x, dy, dw, nullptr, workspace, N, C, K, H, W, hip_stream, stamps);
}
#endif

struct WinoExtras {                       // optional arguments of the general entry point (tai_conv3x3_wino_forward_ex)
    int shift_s = 0;                      // > 0: ONE input tensor read shift_s x shift_s times, displaced by (3a, 3b)
    int zero_tail = 0;                    // the k x k filter's last block has an all-zero third tap row / column (k % 3 != 0)
    int pool_h = 0, pool_w = 0, pool_oy = 0, pool_ox = 0;     // ypool plane and origin (0: H/2 x W/2 at (0, 0))
    const float* addx = nullptr;          // y2 = y + fixed_unpooling(addx)
    float* y2 = nullptr;
};
static int wino_forward_impl(const float* const* xs, int nparts, const float* U, const float* bias, float* y, int N, int C,
                             int K, int H, int W, int act, void* hip_stream, long long* stamps, float* ypool = nullptr,
                             int in_h = 0, int in_w = 0, int in_oy = 0, int in_ox = 0, const WinoExtras& ex = WinoExtras());
static std::atomic<int> g_wino_tall{1};            // 1: use the 128 x 32 workgroup shape when K is a multiple of 128
int tai_conv3x3_wino_set_tall(int on) { return g_wino_tall.exchange(on ? 1 : 0, std::memory_order_relaxed); }
static std::atomic<int> g_wino_timeline_skip{0};   // timeline launches only: loop parts left out (wino_conv.hip.inc, SKIP)
int tai_conv3x3_wino_timeline_skip(int level) {
#ifdef TAI_TIMING_VARIANTS
    g_wino_timeline_skip.store(level, std::memory_order_relaxed);
    return 0;
#else
    if (level == 0) return 0;
    return fail(TAI_SEPCONV_EINVAL, "%s", "timeline skip levels exist only in the tools build (-DTAI_TIMING_VARIANTS)");
#endif
}

int tai_conv3x3_wino_forward(const float* x, const float* U, const float* bias, float* y, int N, int C, int K, int H, int W,
                             int act, void* hip_stream) {
    // (this entry keeps its even-plane contract; odd planes go through tai_conv3x3_wino_forward_ex / _parts)
    if (H % 2 || W % 2) { g_err[0] = 0; return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_forward: needs even H and W (odd planes: _forward_ex, _forward_parts)"); }
    const float* xs[4] = {x, x, x, x};
    return wino_forward_impl(xs, 1, U, bias, y, N, C, K, H, W, act, hip_stream, nullptr);
}

int tai_conv3x3_wino_forward_maxpool(const float* x, const float* U, const float* bias, float* y, float* ypool, int N, int C,
                                     int K, int H, int W, int act, void* hip_stream) {
    if (!ypool) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    const float* xs[4] = {x, x, x, x};
    return wino_forward_impl(xs, 1, U, bias, y, N, C, K, H, W, act, hip_stream, nullptr, ypool);
}

int tai_conv3x3_wino_forward_window(const float* x, const float* U, const float* bias, float* y, float* ypool, int N, int C,
                                    int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, int act, void* hip_stream) {
    const float* xs[4] = {x, x, x, x};
    return wino_forward_impl(xs, 1, U, bias, y, N, C, K, H, W, act, hip_stream, nullptr, ypool, in_h, in_w, in_oy, in_ox);
}

int tai_conv3x3_wino_forward_parts(const float* const* xs, int nparts, const float* U, const float* bias, float* y, int N,
                                   int C, int K, int H, int W, int act, void* hip_stream) {
    if (!xs || nparts < 1 || nparts > 4) return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: 1 to 4 input parts");
    if (nparts > 1 && (C % nparts != 0 || (C / nparts) % 8 != 0))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: parts must have equal channel counts, a multiple of 8");
    const float* p[4];
    for (int i = 0; i < 4; ++i) {
        p[i] = xs[i < nparts ? i : 0];
        if (!p[i]) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    }
    return wino_forward_impl(p, nparts, U, bias, y, N, C, K, H, W, act, hip_stream, nullptr);
}

int tai_conv3x3_wino_forward_timeline(const float* x, const float* U, const float* bias, float* y, int N, int C, int K, int H,
                                      int W, long long* stamps, void* hip_stream) {
    if (!stamps) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    const float* xs[4] = {x, x, x, x};
    return wino_forward_impl(xs, 1, U, bias, y, N, C, K, H, W, 1, hip_stream, stamps);
}

// What tai_conv3x3_wino_forward_ex checks before it builds its WinoExtras, for the entry point and for tai_conv3x3_wino_forward_plan
static int wino_ex_arguments(bool has_xs, int nparts, int shift_k, int C, bool has_addx, bool has_y2) {
    if (!has_xs || nparts < 1 || nparts > 4 || (shift_k != 0 && nparts != 1))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_ex: 1 to 4 input parts, or one tensor read S x S times (shift_k)");
    if (shift_k != 0 && (shift_k < 4 || shift_k > 9))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_ex: shift_k is the size k of the k x k filter, 4 <= k <= 9");
    const int shift_s = shift_k ? (shift_k + 2) / 3 : 0;
    if (nparts > 1 && (C % nparts != 0 || (C / nparts) % 8 != 0))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: parts must have equal channel counts, a multiple of 8");
    if (shift_s != 0 && (C % (shift_s * shift_s) != 0 || (C / (shift_s * shift_s)) % 8 != 0))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_ex: C = S^2 x (a multiple of 8), S = (shift_k + 2) / 3");
    if (has_y2 && !has_addx) return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_ex: y2 needs addx");
    return 0;
}

#ifdef TAI_TIMING_VARIANTS
static long long* g_wino_ex_stamps = nullptr;
int tai_conv3x3_wino_ex_timeline_target(long long* stamps) { g_wino_ex_stamps = stamps; return 0; }
#endif
int tai_conv3x3_wino_forward_ex(const float* const* xs, int nparts, int shift_k, const float* U, const float* bias, float* y,
                                float* ypool, int pool_h, int pool_w, int pool_oy, int pool_ox, const float* addx, float* y2, int N,
                                int C, int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, int act, void* hip_stream) {
    if (int rc = wino_ex_arguments(xs != nullptr, nparts, shift_k, C, addx != nullptr, y2 != nullptr)) return rc;
    const int shift_s = shift_k ? (shift_k + 2) / 3 : 0;
    const float* p[4];
    for (int i = 0; i < 4; ++i) {
        p[i] = xs[i < nparts ? i : 0];
        if (!p[i]) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    }
    WinoExtras ex;
#ifdef TAI_TIMING_VARIANTS
    if (g_wino_ex_stamps && shift_s) {     // tools build: the next displaced-read launch writes timeline stamps (ReLU kernels only)
        ex.shift_s = shift_s; ex.zero_tail = (3 * shift_s > shift_k) ? 1 : 0;
        long long* st = g_wino_ex_stamps;
        g_wino_ex_stamps = nullptr;
        return wino_forward_impl(p, nparts, U, bias, y, N, C, K, H, W, act, hip_stream, st, nullptr, in_h, in_w, in_oy, in_ox, ex);
    }
#endif
    ex.shift_s = shift_s; ex.zero_tail = (shift_k && 3 * shift_s > shift_k) ? 1 : 0; ex.pool_h = pool_h; ex.pool_w = pool_w; ex.pool_oy = pool_oy; ex.pool_ox = pool_ox; ex.addx = addx; ex.y2 = y2;
    return wino_forward_impl(p, nparts, U, bias, y, N, C, K, H, W, act, hip_stream, nullptr, ypool, in_h, in_w, in_oy, in_ox, ex);
}

// THE decisions of one forward launch (wino_forward_impl below, and through it every entry point, and tai_conv3x3_wino_forward_plan): the
// refusals that depend on the dimensions and on which optional arguments are present, then the arithmetic (a buffer made in split
// arithmetic takes the split-bf16 kernel where that kernel has the shape), the workgroup shape, the parts mode, the epilogue and the grid.
// Returns 0, or the refusal (fail).
struct WinoFwdPlan {
    int split, tall, pmode, epi, edge;        // split: 1 = wino::split::conv3x3<A, parts, E, edge>, 0 = wino::conv3x3<ACT, 0, 0, pmode, tall, epi>
    int kblocks, nchunks;                     // blocks of WTM output channels (64; 128 tall), chunks of KC input channels
    long long tblocks, grid;                  // blocks of WTN tiles (64; 32 tall), workgroups
    int in_h, in_w, Kpad, Cpad, cpart, th, tw_all, pool_h, pool_w, pool_oy, pool_ox;
};
static int wino_forward_plan(int nparts, const WinoExtras& ex, bool has_pool, bool has_addx, bool has_y2, bool split_buf, bool stamps, int N, int C,
                             int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, int act, WinoFwdPlan& p) {
    if (in_h == 0) { in_h = H; in_w = W; }
    const int S = ex.shift_s;
    p.in_h = in_h; p.in_w = in_w;
    p.cpart = S ? C / (S * S) : C / nparts;
    const int pool_h = p.pool_h = ex.pool_h ? ex.pool_h : H / 2, pool_w = p.pool_w = ex.pool_h ? ex.pool_w : W / 2;
    const int pool_oy = p.pool_oy = ex.pool_h ? ex.pool_oy : 0, pool_ox = p.pool_ox = ex.pool_h ? ex.pool_ox : 0;
    if (has_pool && (pool_oy < 0 || pool_ox < 0 || pool_h < H / 2 + pool_oy || pool_w < W / 2 + pool_ox))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: bad pooled-output window");
    if (has_pool && (long long)N * K * pool_h * pool_w >= (1LL << 29))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: pooled tensor too large (2^29 elements or more)");
    // displaced reads stay inside the plane: rows up to H + in_oy + 3 (S - 1), columns up to W + 1 + in_ox + 3 (S - 1)
    if (S && (in_oy < 1 || in_ox < 2 || in_h < H + in_oy + 1 + 3 * (S - 1) || in_w < W + in_ox + 2 + 3 * (S - 1)))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_ex: the input plane does not hold the halo of the displaced reads");
    if (N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0 || act < 0 || act > 2)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: bad dimensions, act in {0, 1, 2}");
    // an odd side (the ragged-plane variant, EPI 3 of wino::conv3x3): plain input and output planes only
    const bool ragged = H % 2 != 0 || W % 2 != 0;
    if (ragged && (has_pool || S || has_addx || stamps || in_h != H || in_w != W || in_oy != 0 || in_ox != 0))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: needs even H and W for a pooled output, the unpooling epilogue, an input "
                    "window or displaced reads (odd H or W: plain input and output only)");
    if (in_h < H + in_oy || in_w < W + in_ox || in_oy < 0 || in_ox < 0 || in_ox % 2 || (!ragged && in_w % 2))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: bad input window");
    if ((long long)N * C * in_h * in_w >= (1LL << 29) || (long long)N * K * H * W >= (1LL << 29))   // byte offsets < 2^31
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: tensor too large (2^29 elements or more)");
    p.Kpad = (K + wino::TM - 1) / wino::TM * wino::TM;
    p.Cpad = (C + wino::KC - 1) / wino::KC * wino::KC;
    p.nchunks = p.Cpad / wino::KC;
    p.th = (H + 1) / 2; p.tw_all = (W + 1) / 2;                 // tiles per column / row (ceil: H / 2, W / 2 on even planes)
    const long long tiles = (long long)N * p.th * p.tw_all;
    const int epi = has_addx ? (has_y2 ? 1 : 2) : 0;
    // A buffer made in split arithmetic (tai_conv3x3_wino_set_arithmetic(1)) takes the split-bf16 kernel where that kernel has the
    // shape: no displaced reads, no timeline stamps, tile rows of 2^k or 16 m tiles (its 16-lane neighbour shifts).
    if (split_buf && ragged)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino: the split-bf16 arithmetic needs even H and W");
    const int tw = W / 2;
    const bool tw_ok = tw % 16 == 0 || (tw >= 2 && (tw & (tw - 1)) == 0);
    if (split_buf && !S && !stamps && tw_ok && !(epi && act != 0)) {
        p.split = 1; p.tall = 0; p.pmode = nparts > 1 ? 1 : 0; p.epi = epi;
        p.edge = tw > 16 || in_ox > 0 || in_w > W + in_ox;
        p.kblocks = p.Kpad / wino::TM;
        p.tblocks = (tiles + wino::TN - 1) / wino::TN;
        p.grid = p.tblocks * p.kblocks;
        return 0;
    }
    // 128-channel x 32-tile workgroups (half the patch transform and LDS writes per MFMA) where K allows
    p.split = 0; p.edge = 0;
    p.tall = p.Kpad % wino::TTM == 0 && g_wino_tall.load(std::memory_order_relaxed) != 0;
    p.pmode = S ? 2 : (nparts > 1 ? 1 : 0);
    // the instantiations the path uses: the second-output / sum epilogues come without activation (Residual's last
    // convolution) on one tensor or cat operands; the displaced reads come with ReLU (MotionEnc)
    if (epi && (act != 0 || p.pmode == 2 || stamps)) return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_ex: addx needs act 0 and no displaced reads");
    if (p.pmode == 2 && act != 1) return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino_ex: displaced reads are built for act 1 (ReLU)");
    p.epi = epi ? epi : (ragged ? 3 : 0);
    p.kblocks = p.tall ? p.Kpad / wino::TTM : p.Kpad / wino::TM;
    p.tblocks = p.tall ? (tiles + wino::TTN - 1) / wino::TTN : (tiles + wino::TN - 1) / wino::TN;
    p.grid = p.tblocks * p.kblocks;
    return 0;
}

// The plan of a launch as a query: the argument checks of tai_conv3x3_wino_forward_ex (wino_ex_arguments) and the same wino_forward_plan
// call as the launcher makes, hence the same refusals with the same words.  The pooled output, where asked for, is the plain
// [N, K, H/2, W/2] tensor.  U: the transformed-weight buffer the launch would read (its recorded arithmetic decides), or NULL for a
// buffer in fp32 arithmetic.  No stream, no launch.
int tai_conv3x3_wino_forward_plan(int nparts, int shift_k, int has_pool, int has_addx, int has_y2, int N, int C, int K, int H, int W, int in_h,
                                  int in_w, int in_oy, int in_ox, int act, const float* U, int* out) {
    g_err[0] = 0;
    if (!out) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    if (int rc = wino_ex_arguments(true, nparts, shift_k, C, has_addx != 0, has_y2 != 0)) return rc;
    WinoExtras ex;
    ex.shift_s = shift_k ? (shift_k + 2) / 3 : 0;
    ex.zero_tail = (shift_k && 3 * ex.shift_s > shift_k) ? 1 : 0;
    bool split_buf = false;
    if (U) { std::lock_guard<std::mutex> lk(g_split_mu); split_buf = g_split_bufs.count(U) != 0; }
    WinoFwdPlan p;
    if (int rc = wino_forward_plan(nparts, ex, has_pool != 0, has_addx != 0, has_y2 != 0, split_buf, false, N, C, K, H, W, in_h, in_w, in_oy, in_ox, act, p))
        return rc;
    const int v[9] = {p.split, p.tall, p.pmode, p.epi, p.edge, p.kblocks, (int)p.tblocks, p.nchunks, (int)p.grid};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
    return (int)p.grid;
}

static int wino_forward_impl(const float* const* xs, int nparts, const float* U, const float* bias, float* y, int N, int C,
                             int K, int H, int W, int act, void* hip_stream, long long* stamps, float* ypool, int in_h,
                             int in_w, int in_oy, int in_ox, const WinoExtras& ex) {
    g_err[0] = 0;
    if (!xs[0] || !U || !bias || !y) return fail(TAI_SEPCONV_EINVAL, "%s", "null pointer");
    bool split_buf;
    { std::lock_guard<std::mutex> lk(g_split_mu); split_buf = g_split_bufs.count(U) != 0; }
    WinoFwdPlan p;
    if (int rc = wino_forward_plan(nparts, ex, ypool != nullptr, ex.addx != nullptr, ex.y2 != nullptr, split_buf, stamps != nullptr, N, C, K, H, W, in_h,
                                   in_w, in_oy, in_ox, act, p))
        return rc;
    in_h = p.in_h; in_w = p.in_w;
    const int S = ex.shift_s, cpart = p.cpart, Kpad = p.Kpad, nchunks = p.nchunks;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    // the divisors of the kernels' index arithmetic: tiles per image, tiles per row, blocks of output channels
    wino::DivMagic dv;
    wino_div_magic((long long)p.th * p.tw_all, dv.m_tpi, dv.s_tpi);
    wino_div_magic(p.tw_all, dv.m_tw, dv.s_tw);
    wino_div_magic(p.kblocks, dv.m_kb, dv.s_kb);
    if (p.split) {
        const unsigned short* U3 = reinterpret_cast<const unsigned short*>(U + 16LL * Kpad * p.Cpad);
        const bool edge = p.edge != 0, parts = p.pmode == 1;
        auto kern = p.epi == 1 ? wino_split_kernel<0, 1>(parts, edge) : p.epi == 2 ? wino_split_kernel<0, 2>(parts, edge)
                  : act == 0 ? wino_split_kernel<0, 0>(parts, edge) : act == 1 ? wino_split_kernel<1, 0>(parts, edge)
                                                                               : wino_split_kernel<2, 0>(parts, edge);
        if (int rc = launch(kern, dim3((unsigned)p.grid), dim3(512), wino::split::LDS_BYTES, s, xs[0], xs[1], xs[2], xs[3], cpart, U3,
                            bias, y, ypool, N, C, K, H, W, in_h, in_w, in_oy, in_ox, nchunks, p.kblocks, p.pool_h, p.pool_w, p.pool_oy, p.pool_ox, ex.addx,
                            ex.y2, dv, nullptr))
            return rc;
        return check_launch("conv3x3_wino_split");
    }
    const bool tall = p.tall != 0;
    const int pmode = p.pmode;
    const int part_magic = S ? (1 << 20) / (cpart / 8) + 1 : 0;     // chunk -> channel block of the displaced reads
    WinoKernel kern;        // <ACT, DBG, SKIP, PARTS, TALL, EPI>
    if (stamps) {           // timeline launches (tools/wino_timeline.py): ReLU, one tensor
        kern = wino_kernel<1, 1, 0, 0, 0>(tall);
#ifdef TAI_TIMING_VARIANTS
        const int skip = g_wino_timeline_skip.load(std::memory_order_relaxed);
        if (skip == 1) kern = wino_kernel<1, 1, 1, 0, 0>(tall);
        else if (skip == 2) kern = wino_kernel<1, 1, 2, 0, 0>(tall);
        else if (skip == 4) kern = wino_kernel<1, 1, 4, 0, 0>(tall);
        else if (skip == 5) kern = wino_kernel<1, 1, 5, 0, 0>(tall);
        else if (skip == 7) kern = wino_kernel<1, 2, 0, 0, 0>(tall);
        else if (pmode == 2) kern = wino_kernel<1, 1, 0, 2, 0>(tall);
#endif
    }
    else if (p.epi == 1) kern = pmode == 1 ? wino_kernel<0, 0, 0, 1, 1>(tall) : wino_kernel<0, 0, 0, 0, 1>(tall);
    else if (p.epi == 2) kern = pmode == 1 ? wino_kernel<0, 0, 0, 1, 2>(tall) : wino_kernel<0, 0, 0, 0, 2>(tall);
    else if (pmode == 2) kern = wino_kernel<1, 0, 0, 2, 0>(tall);
    else if (p.epi == 3) kern = pmode == 1 ? wino_kernel_act<1, 3>(act, tall) : wino_kernel_act<0, 3>(act, tall);       // odd H or W
    else kern = pmode == 1 ? wino_kernel_act<1, 0>(act, tall) : wino_kernel_act<0, 0>(act, tall);
    if (int rc = launch(kern, dim3((unsigned)p.grid), dim3(256), tall ? wino::TLDS_BYTES : wino::LDS_BYTES, s, xs[0], xs[1], xs[2], xs[3], cpart, U, bias, y,
                        ypool, N, C, K, H, W, in_h, in_w, in_oy, in_ox, Kpad, nchunks, p.kblocks, stamps, p.pool_h, p.pool_w, p.pool_oy, p.pool_ox, ex.addx,
                        ex.y2, S, part_magic, ex.zero_tail, dv))
        return rc;
    return check_launch("conv3x3_wino");
}

}  // extern "C"
