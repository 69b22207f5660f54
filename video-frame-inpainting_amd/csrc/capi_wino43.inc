// Winograd F(4x4, 3x3) entry points (included by sepconv_capi.hip, before capi_wino.inc).

extern "C" {

// ---- Winograd F(4x4, 3x3) on the fp32 MFMA pipe (csrc/wino43_conv.hip.inc): opt-in prototype -------------------------------------
long long tai_conv3x3_wino43_weight_floats(int K, int C) {
    if (K <= 0 || C <= 0) return 0;
    const long long Kpad = (K + wino43::TM - 1) / wino43::TM * wino43::TM;
    const long long Cpad = (C + wino43::KC - 1) / wino43::KC * wino43::KC;       // zero weights for the channels past C
    return 36 * Kpad * Cpad;
}

int tai_conv3x3_wino43_transform_weights(const float* weight, float* U, int K, int C, void* hip_stream) {
    g_err[0] = 0;
    if (!weight || !U || K <= 0 || C <= 0)
        return fail(TAI_SEPCONV_EINVAL, "%s", "wino43 transform_weights: bad argument");
    const int Kpad = (K + wino43::TM - 1) / wino43::TM * wino43::TM;
    const int Cpad = (C + wino43::KC - 1) / wino43::KC * wino43::KC;
    const long long total = (long long)Kpad * Cpad;
    hipLaunchKernelGGL(wino43::transform_weights, dim3(grid_for(total, 4096)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), weight, U, K, C,
                       Kpad, Cpad);
    return check_launch("wino43_transform_weights");
}

// 0: the kernel (generated chunk loop); 101..112 (tools build only): timing ablations / schedule variants of it.  Round 4's compiler-
// scheduled forms (waves 8 / 4) are gone with their transform constants (profiles/r04_wino43_prototype.txt, r05_wino43_forms.txt keep the A/B).
static std::atomic<int> g_wino43_waves{0};
int tai_conv3x3_wino43_set_waves(int waves) {
#ifdef TAI_TIMING_VARIANTS   // (timing only, wrong results; tools/gen_wino43_asm.py ABLATIONS)
    if (waves >= 101 && waves <= 112) return g_wino43_waves.exchange(waves, std::memory_order_relaxed);
#endif
    if (waves != 0) return -1;
    return g_wino43_waves.exchange(waves, std::memory_order_relaxed);
}

// Workgroup placement of the F(4x4, 3x3) kernels (forward and weight gradient): 1 (default) = aware of the 8 XCDs and their L2s (see
// conv3x3_gen / conv3x3_wrw_gen), 0 = the dispatch order of rounds 4-5.  Same results either way; for A/B timing.
static std::atomic<int> g_wino43_placement{1};
int tai_conv3x3_wino43_set_placement(int xcd_aware) { return g_wino43_placement.exchange(xcd_aware ? 1 : 0, std::memory_order_relaxed); }

// Split of the forward's reduction over input channels (tai_conv3x3_wino43_forward_ws, wino43::conv3x3_gen<..., SPLITC>): 1 (default) =
// where the grid of 64-channel x 32-tile workgroups leaves CUs idle, 0 = never (the dispatch of round 5).  For A/B timing.
static std::atomic<int> g_wino43_splitc{1};
int tai_conv3x3_wino43_set_splitc(int on) { return g_wino43_splitc.exchange(on ? 1 : 0, std::memory_order_relaxed); }

// The split count.  A workgroup holds a CU (108 KB of LDS), so a grid of B workgroups runs in ceil(B / 256) rounds; with S splits of c
// chunks each it runs ceil(B S / 256) rounds of c chunks, and every split writes its partial tiles and the reduction reads them back.
// Cost in chunk times of a full round: ceil(B S / 256) (c + 2) (+2: the loop's fill and the inverse transform) plus, for S > 1,
// B (2 S + 1) / 64 (the partials of a workgroup, 128 KB, are ~1/64 of a chunk time of the whole chip in memory traffic, written once and
// read once, plus the final write).  The cheapest S wins if it saves 5 % on S = 1; large grids keep S = 1.  Splits hold at least
// W43_MIN_SPLIT_CHUNKS chunks and break on part boundaries (the chunks of a split lie in one part, or are whole parts).
struct W43Split { int splits, chunks_per_split; };
constexpr int W43_MIN_SPLIT_CHUNKS = 8, W43_MAX_SPLITS = 16;
static W43Split wino43_split_plan(int N, int C, int K, int H, int W, int nparts) {
    const int nchunks = C > 0 ? (C + wino43::KC - 1) / wino43::KC : 0;
    const W43Split one{1, nchunks};
    if (!g_wino43_splitc.load(std::memory_order_relaxed) || N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0 || H % 4 != 0 || W % 4 != 0 ||
        nparts < 1 || nparts > 4 || C % nparts != 0 || (nparts > 1 && (C / nparts) % wino43::KC != 0))
        return one;
    const int cpp = nparts == 1 ? nchunks : C / nparts / wino43::KC;
    const long long blocks = ((long long)N * (H / 4) * (W / 4) + wino43::TN - 1) / wino43::TN * ((K + wino43::TM - 1) / wino43::TM);
    auto cost = [&](int sp, int cps) {
        return (double)((blocks * sp + 255) / 256) * (cps + 2) + (sp > 1 ? (double)blocks * (2 * sp + 1) / 64.0 : 0.0);
    };
    const double c1 = cost(1, nchunks);
    double best = c1;
    W43Split pick = one;
    for (int want = 2; want <= W43_MAX_SPLITS; ++want) {
        int cps = (nchunks + want - 1) / want;
        if (nparts > 1) {
            if (cps < cpp) { while (cpp % cps != 0) ++cps; }       // a divisor of the part's chunks ...
            else cps = (cps + cpp - 1) / cpp * cpp;                 // ... or whole parts
        }
        if (cps < W43_MIN_SPLIT_CHUNKS) break;
        const int sp = (nchunks + cps - 1) / cps;
        if (sp < 2) continue;
        const double c = cost(sp, cps);
        if (c < best) { best = c; pick = W43Split{sp, cps}; }
    }
    return best <= 0.95 * c1 ? pick : one;
}

int tai_conv3x3_wino43_splits(int N, int C, int K, int H, int W, int nparts, int* chunks_per_split) {
    const W43Split sc = wino43_split_plan(N, C, K, H, W, nparts);
    if (chunks_per_split) *chunks_per_split = sc.chunks_per_split;
    return sc.splits;
}

long long tai_conv3x3_wino43_workspace_floats(int N, int C, int K, int H, int W, int nparts) {
    const W43Split sc = wino43_split_plan(N, C, K, H, W, nparts);
    return sc.splits > 1 ? (long long)sc.splits * N * K * H * W : 0;
}

// The (ACT, EPI) instance of an F(4x4, 3x3) kernel that serves (act, ypool, addx, y2), as the index into a table of instances in the
// order <0, 0>, <1, 0>, <0, 1>, <1, 1>, <2, 0>, <0, 2>, <0, 3>: EPI 1 writes the pooled second output, 2 writes y2 = y + unpool(addx),
// 3 adds unpool(addx) into y.  (The callers have refused the combinations that have no instance.)
constexpr int W43_INSTANCES = 7;
static int wino43_instance(int act, const float* ypool, const float* addx, const float* y2) {
    if (ypool) return act == 0 ? 2 : 3;
    if (addx) return y2 ? 5 : 6;
    return act == 2 ? 4 : act;
}

// One launch of an instance of wino43::conv3x3_gen: a workgroup per block of 64 output channels x 32 tiles and split
using W43Kernel = decltype(&wino43::conv3x3_gen<0, 0>);
static int launch_gen(W43Kernel kern, int splits, hipStream_t s, const float* const* p, int cpart, const float* U, const float* bias, float* y,
                      int N, int C, int K, int H, int W, float* ypool, const float* addx, float* y2, const wino43::Window& win) {
    const int Kpad = (K + wino43::TM - 1) / wino43::TM * wino43::TM;
    const int kblocks = Kpad / wino43::TM, nchunks = (C + wino43::KC - 1) / wino43::KC;
    const long long tiles = (long long)N * (H / 4) * (W / 4);
    const long long tblocks = (tiles + wino43::TN - 1) / wino43::TN;
    return launch(kern, dim3((unsigned)(tblocks * kblocks * splits)), dim3(512), wino43::LDS_BYTES, s, p[0], p[1], p[2], p[3], cpart, U, bias, y, N, C, K,
                  H, W, Kpad, nchunks, kblocks, ypool, addx, y2, win);
}

// ws_floats < 0: the entry points without a workspace (never split); else tai_conv3x3_wino43_forward_ws
static int wino43_forward_impl(const float* const* xs, int nparts, const float* U, const float* bias, float* y, int N, int C, int K, int H,
                               int W, int act, void* hip_stream, float* ypool = nullptr, const float* addx = nullptr, float* y2 = nullptr,
                               float* ws = nullptr, long long ws_floats = -1) {
    if (!xs || !xs[0] || !U || !bias || !y || N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0 || nparts < 1 || nparts > 4)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43: bad argument (1 to 4 input parts)");
    // one tensor: any C (the transformed weights of the channels past C are zero and the loads of those channels past the tensor's end
    // return 0; inside it they read the next image's first channels, finite values times zero)
    const bool ragged = nparts == 1 && C % wino43::KC != 0;
    if (H % 4 != 0 || W % 4 != 0 || C % nparts != 0 || (!ragged && (C / nparts) % wino43::KC != 0) || act < 0 || act > 2)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43: needs H and W multiples of 4, the channels of a part a multiple of 4 (any C for one part), act in {0, 1, 2}");
    if ((long long)N * C * H * W >= (1LL << 29) || (long long)N * K * H * W >= (1LL << 29))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43: tensor too large (2^29 elements or more)");
    if ((y2 && !addx) || (addx && (act != 0 || ypool)) || (ypool && act == 2))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43_ex: y2 needs addx; addx needs act 0 and no pooled output; no pooled output with tanh");
    const float* p[4] = {xs[0], xs[0], xs[0], xs[0]};
    for (int i = 0; i < nparts; ++i) {
        if (!xs[i]) return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43: null input part");
        p[i] = xs[i];
    }
    const int nchunks = (C + wino43::KC - 1) / wino43::KC, cpart = C / nparts;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    wino43::Window plain_win{};
    plain_win.dispatch_order = g_wino43_placement.load(std::memory_order_relaxed) ? 0 : 1;
#ifdef TAI_TIMING_VARIANTS
    const int var = g_wino43_waves.load(std::memory_order_relaxed);
    if (var >= 101 && var <= 112) {      // ablation VAR = 1 .. 12 of the ReLU kernel
        static const W43Kernel ablations[12] = {
            wino43::conv3x3_gen<1, 0, 1>, wino43::conv3x3_gen<1, 0, 2>, wino43::conv3x3_gen<1, 0, 3>, wino43::conv3x3_gen<1, 0, 4>,
            wino43::conv3x3_gen<1, 0, 5>, wino43::conv3x3_gen<1, 0, 6>, wino43::conv3x3_gen<1, 0, 7>, wino43::conv3x3_gen<1, 0, 8>,
            wino43::conv3x3_gen<1, 0, 9>, wino43::conv3x3_gen<1, 0, 10>, wino43::conv3x3_gen<1, 0, 11>, wino43::conv3x3_gen<1, 0, 12>};
        if (int rc = launch_gen(ablations[var - 101], 1, s, p, cpart, U, bias, y, N, C, K, H, W, ypool, addx, y2, plain_win)) return rc;
        return check_launch("conv3x3_wino43 (ablation)");
    }
#endif
    static const W43Kernel plain[W43_INSTANCES] = {wino43::conv3x3_gen<0, 0>, wino43::conv3x3_gen<1, 0>, wino43::conv3x3_gen<0, 1>, wino43::conv3x3_gen<1, 1>,
                                                   wino43::conv3x3_gen<2, 0>, wino43::conv3x3_gen<0, 2>, wino43::conv3x3_gen<0, 3>};
    const int inst = wino43_instance(act, ypool, addx, y2);
    const W43Split sc = ws_floats >= 0 ? wino43_split_plan(N, C, K, H, W, nparts) : W43Split{1, nchunks};
    if (sc.splits > 1) {
        if (!ws || ws_floats < (long long)sc.splits * N * K * H * W)
            return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43_forward_ws: workspace missing or smaller than tai_conv3x3_wino43_workspace_floats");
        wino43::Window win = plain_win;
        win.splits = sc.splits;
        win.chunks_per_split = sc.chunks_per_split;
        if (int rc = launch_gen(wino43::conv3x3_gen<0, 0, 0, false, true>, sc.splits, s, p, cpart, U, bias, ws, N, C, K, H, W, nullptr, nullptr, nullptr, win))
            return rc;
        if (int rc = check_launch("conv3x3_wino43 (split over input channels)")) return rc;
        static const decltype(&wino43::splitc_reduce<0, 0>) reduce[W43_INSTANCES] = {
            wino43::splitc_reduce<0, 0>, wino43::splitc_reduce<1, 0>, wino43::splitc_reduce<0, 1>, wino43::splitc_reduce<1, 1>,
            wino43::splitc_reduce<2, 0>, wino43::splitc_reduce<0, 2>, wino43::splitc_reduce<0, 3>};
        const long long work = (long long)N * K * (H / 4) * (W / 4);
        hipLaunchKernelGGL(reduce[inst], dim3(grid_for(work, 65536)), dim3(256), 0, s, ws, sc.splits, bias, y, N, K, H, W, ypool, addx, y2);
        return check_launch("conv3x3_wino43_splitc_reduce");
    }
    if (int rc = launch_gen(plain[inst], 1, s, p, cpart, U, bias, y, N, C, K, H, W, ypool, addx, y2, plain_win)) return rc;
    return check_launch("conv3x3_wino43");
}

int tai_conv3x3_wino43_forward(const float* x, const float* U, const float* bias, float* y, int N, int C, int K, int H, int W, int act,
                               void* hip_stream) {
    g_err[0] = 0;
    const float* xs[1] = {x};
    return wino43_forward_impl(xs, 1, U, bias, y, N, C, K, H, W, act, hip_stream);
}

int tai_conv3x3_wino43_forward_parts(const float* const* xs, int nparts, const float* U, const float* bias, float* y, int N, int C, int K,
                                     int H, int W, int act, void* hip_stream) {
    g_err[0] = 0;
    return wino43_forward_impl(xs, nparts, U, bias, y, N, C, K, H, W, act, hip_stream);
}

int tai_conv3x3_wino43_forward_ex(const float* const* xs, int nparts, const float* U, const float* bias, float* y, float* ypool,
                                  const float* addx, float* y2, int N, int C, int K, int H, int W, int act, void* hip_stream) {
    g_err[0] = 0;
    return wino43_forward_impl(xs, nparts, U, bias, y, N, C, K, H, W, act, hip_stream, ypool, addx, y2);
}

int tai_conv3x3_wino43_forward_ws(const float* const* xs, int nparts, const float* U, const float* bias, float* y, float* ypool,
                                  const float* addx, float* y2, float* workspace, long long workspace_floats, int N, int C, int K, int H,
                                  int W, int act, void* hip_stream) {
    g_err[0] = 0;
    if (workspace_floats < 0) return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43_forward_ws: negative workspace size");
    return wino43_forward_impl(xs, nparts, U, bias, y, N, C, K, H, W, act, hip_stream, ypool, addx, y2, workspace, workspace_floats);
}

int tai_conv3x3_wino43_forward_blocks(const float* x, int shift_k, const float* U, const float* bias, float* y, float* ypool, int pool_h,
                                      int pool_w, int pool_oy, int pool_ox, int N, int C, int K, int H, int W, int in_h, int in_w, int in_oy,
                                      int in_ox, int act, void* hip_stream) {
    g_err[0] = 0;
    const int S = (shift_k + 2) / 3;
    if (!x || !U || !bias || !y || N <= 0 || C <= 0 || K <= 0 || H <= 0 || W <= 0 || shift_k < 4 || shift_k > 9 || C % (S * S) != 0 ||
        (C / (S * S)) % wino43::KC != 0 || H % 4 != 0 || W % 4 != 0 || act < 0 || act > 1)
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43_blocks: bad argument (4 <= shift_k <= 9, C = S^2 x a multiple of 4, H and W multiples of 4, act 0 / 1)");
    // every read of every block must lie inside the plane: rows in_oy - 1 ... in_oy + H + 3 (S - 1), columns in_ox - 1 ... in_ox + W + 3 (S - 1)
    if (in_oy < 1 || in_ox < 1 || in_h < in_oy + H + 1 + 3 * (S - 1) || in_w < in_ox + W + 1 + 3 * (S - 1))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43_blocks: the input plane does not carry the halo the displaced reads need");
    const int cin = C / (S * S);
    if ((long long)N * cin * in_h * in_w >= (1LL << 29) || (long long)N * K * H * W >= (1LL << 29))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43_blocks: tensor too large (2^29 elements or more)");
    if (ypool && pool_h > 0 && (pool_w % 2 != 0 || pool_ox % 2 != 0 || pool_oy < 0 || pool_ox < 0 || pool_oy + H / 2 > pool_h || pool_ox + W / 2 > pool_w))
        return fail(TAI_SEPCONV_EINVAL, "%s", "conv3x3_wino43_blocks: the pooled-output window must be even in pool_w and pool_ox and lie inside its plane");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const wino43::Window win{in_h, in_w, in_oy, in_ox, S, ypool ? pool_h : 0, pool_w, pool_oy, pool_ox, 3 * S > shift_k ? 1 : 0,
                             g_wino43_placement.load(std::memory_order_relaxed) ? 0 : 1};
    // (act 0 / 1 and no unpooling epilogue: the first four instances)
    static const W43Kernel blocks[4] = {wino43::conv3x3_gen<0, 0, 0, true>, wino43::conv3x3_gen<1, 0, 0, true>, wino43::conv3x3_gen<0, 1, 0, true>,
                                        wino43::conv3x3_gen<1, 1, 0, true>};
    const float* p[4] = {x, x, x, x};
    if (int rc = launch_gen(blocks[wino43_instance(act, ypool, nullptr, nullptr)], 1, s, p, cin, U, bias, y, N, C, K, H, W, ypool, nullptr, nullptr, win))
        return rc;
    return check_launch("conv3x3_wino43_blocks");
}

}  // extern "C"
