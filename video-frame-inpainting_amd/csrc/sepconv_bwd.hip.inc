// Backward kernels of the adaptive separable convolution (included by sepconv_capi.hip).
//
// Replace kernel_SeparableConvolution_updateGradV / updateGradH / updateGradI
// (reference src/separable_convolution/cfile/SeparableConvolution_kernel.cu:49-86, :88-118, :120-162).
//
//   gV[b,fy,y,x] = sum_c gO[b,c,y,x] * sum_fx in[b,c,y+fy,x+fx] h[b,fx,y,x]
//   gH[b,fx,y,x] = sum_c gO[b,c,y,x] * sum_fy in[b,c,y+fy,x+fx] v[b,fy,y,x]
//   gI[b,c,Y,X]  = sum_{fy,fx} gO[b,c,Y-fy,X-fx] v[b,fy,Y-fy,X-fx] h[b,fx,Y-fy,X-fx]
//
// gV and gH reuse the forward kernel's tiling (input patch in LDS, a lane owns 4 adjacent pixels,
// every tap-plane access is a 16-byte load or store per lane):
//   * gV keeps the horizontal taps register-resident, forms the same per-row sums r[fy] as the
//     forward pass and STORES gO*r[fy] for each fy instead of folding it with v;
//   * gH keeps ks float4 ACCUMULATORS register-resident (one per horizontal tap), streams v one
//     plane per row, and stores the accumulators once at the end.
// gI is a scatter (no operand reuse exists in gather form: each term needs v and h of a different
// pixel); this first version runs the bounds-checked gather of the reference with coalesced reads
// and the channel loop innermost so v and h are fetched once per tap for all channels.

namespace bwd {

using fwd::Cfg;
using fwd::TILE_W;
using fwd::comp;

template <int KS, int NC>
__device__ __forceinline__ void stage_patch(float* patch, const float* __restrict__ in, int b, int C,
                                            int Hp, int Wp, int y0, int x0, int tid) {
    using K = Cfg<KS, 1>;
    for (int c = 0; c < NC; ++c) {
        const float* src = in + ((size_t)(b * C + c) * Hp) * Wp;
        float* dst = patch + c * K::PR * K::PITCH;
        for (int idx = tid; idx < K::PR * K::PC; idx += K::THREADS) {
            const int r = idx / K::PC, cc = idx - r * K::PC;
            const int gy = min(y0 + r, Hp - 1), gx = min(x0 + cc, Wp - 1);
            dst[r * K::PITCH + cc] = src[(size_t)gy * Wp + gx];
        }
    }
}

// gH epilogue of the accumulator-resident wave type: gH[t] = gO * c[t], one 16-byte store per tap plane
template <int T>
__device__ __forceinline__ void store_scaled_taps(float* dst, const fwd::TapRegs& c, const float4& go, size_t plane) {
    if constexpr (T < 51) {
        *reinterpret_cast<float4*>(dst + (size_t)T * plane) =
            make_float4(go.x * fwd::tap_get<T>(c), go.y * fwd::tap_get<51 + T>(c), go.z * fwd::tap_get<102 + T>(c),
                        go.w * fwd::tap_get<153 + T>(c));
        store_scaled_taps<T + 1>(dst, c, go, plane);
    }
}

template <int KS, int NC>
__global__ __launch_bounds__((Cfg<KS, 1>::THREADS), 2)
void sepconv_grad_v_tiled(const float* __restrict__ gO, const float* __restrict__ in,
                          const float* __restrict__ ht, float* __restrict__ gV, int H, int W,
                          int tiles_x, int tiles_y) {
    using K = Cfg<KS, 1>;
    extern __shared__ __attribute__((aligned(16))) float patch[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = fwd::xcd_contiguous_block_id();
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int x0 = tx * TILE_W, y0 = ty * K::TILE_H;
    const int Hp = H + KS - 1, Wp = W + KS - 1;
    stage_patch<KS, NC>(patch, in, b, NC, Hp, Wp, y0, x0, tid);

    const int g = lane & 31, ly = wave * 2 + (lane >> 5);
    const int y = y0 + ly, x = x0 + 4 * g;
    const bool active = (y < H) && (x < W);
    const int yc = min(y, H - 1), xc = min(x, W - 4);
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)yc * W + xc;
    const float* hp = ht + ((size_t)b * KS) * plane + pix;

    float4 hq[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t) hq[t] = *reinterpret_cast<const float4*>(hp + (size_t)t * plane);
    float4 go[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        go[c] = *reinterpret_cast<const float4*>(gO + ((size_t)(b * NC + c)) * plane + pix);

    __syncthreads();
    const float* rowbase = patch + ly * K::PITCH + 4 * g;
    float* gvp = gV + ((size_t)b * KS) * plane + pix;
#pragma unroll 1
    for (int fy = 0; fy < KS; ++fy) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float4* rowp =
                reinterpret_cast<const float4*>(rowbase + c * K::PR * K::PITCH + fy * K::PITCH);
            float r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < K::NCHUNK; ++k) {
                const float4 w = rowp[k];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int t = 4 * k + i - p;
                        if (t >= 0 && t < KS) r[p] = fmaf(comp(hq[t], p), comp(w, i), r[p]);
                    }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) s[p] = fmaf(comp(go[c], p), r[p], s[p]);
        }
        if (active)
            *reinterpret_cast<float4*>(gvp + (size_t)fy * plane) = make_float4(s[0], s[1], s[2], s[3]);
    }
}

template <int KS, int NC>
__global__ __launch_bounds__((Cfg<KS, 1>::THREADS), 2)
void sepconv_grad_h_tiled(const float* __restrict__ gO, const float* __restrict__ in,
                          const float* __restrict__ vt, float* __restrict__ gH, int H, int W,
                          int tiles_x, int tiles_y) {
    using K = Cfg<KS, 1>;
    extern __shared__ __attribute__((aligned(16))) float patch[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = fwd::xcd_contiguous_block_id();
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int x0 = tx * TILE_W, y0 = ty * K::TILE_H;
    const int Hp = H + KS - 1, Wp = W + KS - 1;
    stage_patch<KS, NC>(patch, in, b, NC, Hp, Wp, y0, x0, tid);

    const int g = lane & 31, ly = wave * 2 + (lane >> 5);
    const int y = y0 + ly, x = x0 + 4 * g;
    const bool active = (y < H) && (x < W);
    const int yc = min(y, H - 1), xc = min(x, W - 4);
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)yc * W + xc;
    const float* vp = vt + ((size_t)b * KS) * plane + pix;

    float4 go[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        go[c] = *reinterpret_cast<const float4*>(gO + ((size_t)(b * NC + c)) * plane + pix);

    float acc[KS][4];
#pragma unroll
    for (int t = 0; t < KS; ++t)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[t][p] = 0.f;

    __syncthreads();
    const float* rowbase = patch + ly * K::PITCH + 4 * g;
    float4 vnext = *reinterpret_cast<const float4*>(vp);
#pragma unroll 1
    for (int fy = 0; fy < KS; ++fy) {
        const float4 vv = vnext;
        vnext = *reinterpret_cast<const float4*>(vp + (size_t)min(fy + 1, KS - 1) * plane);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float a[4] = {go[c].x * vv.x, go[c].y * vv.y, go[c].z * vv.z, go[c].w * vv.w};
            const float4* rowp =
                reinterpret_cast<const float4*>(rowbase + c * K::PR * K::PITCH + fy * K::PITCH);
#pragma unroll
            for (int k = 0; k < K::NCHUNK; ++k) {
                const float4 w = rowp[k];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int t = 4 * k + i - p;
                        if (t >= 0 && t < KS) acc[t][p] = fmaf(a[p], comp(w, i), acc[t][p]);
                    }
            }
        }
    }
    if (active) {
        float* ghp = gH + ((size_t)b * KS) * plane + pix;
#pragma unroll
        for (int t = 0; t < KS; ++t)
            *reinterpret_cast<float4*>(ghp + (size_t)t * plane) =
                make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
}

// ---- gV and gH in one launch, single channel: the forward's two hand-scheduled wave types --------------------------
// An 8-wave workgroup owns 8 rows x 128 columns.  Waves 0-3 are the forward's type B with the roles renamed: they keep
// c[fx] = sum_fy v[fy] * in[y+fy, x+fx] register-resident, stream v from the first microsecond and finish with
// gH[fx] = gO * c[fx] (51 16-byte stores).  Waves 4-7 own the SAME pixels as type A without a v stream: taps
// register-resident, one 16-byte store of gV[fy] = gO * r[fy] per row.  Wave w and w+4 share a SIMD, so the tap loads of
// the gV wave hide under the gH wave's FMAs, and the two 107 MB write streams interleave with the two 107 MB reads.
// EARLY (default): as the forward kernel 18 -- the gV waves issue their 51 tap loads at kernel entry, the patch is staged by the
// four gH waves alone (LDS-DMA) and announced through an LDS counter that every wave polls before its first patch read; no
// workgroup barrier stands between a gV wave and its tap loads.
// GVP: priority of the gV waves in their row loop (0: never set; the gH waves sit at 1).
// Either output may be null: its four waves then leave before their row loop (the gH waves still stage the patch), so a
// gradient carries the same bits whether or not the other one was requested.
template <bool EARLY, int GVP = 0>
__global__ __launch_bounds__(512, 2)
void sepconv_grad_vh_ab(const float* __restrict__ gO, const float* __restrict__ in, const float* __restrict__ vt,
                        const float* __restrict__ ht, float* __restrict__ gV, float* __restrict__ gH, int H, int W,
                        int tiles_x, int tiles_y) {
    constexpr int KS = 51, THREADS = 512, TILE_H = 8;
    constexpr int PR = TILE_H + KS - 1;
    constexpr int PATCH_BYTES = (PR * 180 * 4 + 1023) & ~1023;
    extern __shared__ __attribute__((aligned(16))) float patch[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = fwd::xcd_contiguous_block_id();
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int x0 = tx * TILE_W, y0 = ty * TILE_H;
    const int Hp = H + KS - 1, Wp = W + KS - 1;
    if constexpr (!EARLY) fwd::stage_patch_vec4<PR, THREADS>(patch, in + ((size_t)b * Hp) * Wp, Hp, Wp, y0, x0, tid);

    const bool is_gh = wave < 4;
    const int g = lane & 31;
    const int ly = (wave & 3) * 2 + (lane >> 5);
    const int y = y0 + ly, x = x0 + 4 * g;
    const bool active = (y < H) && (x < W);
    const int yc = min(y, H - 1), xc = min(x, W - 4);
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)yc * W + xc;
    const unsigned goff = (unsigned)(pix * sizeof(float));
    const unsigned row_addr = (unsigned)((ly * 180 + 4 * g) * sizeof(float));
    const unsigned plane_bytes = (unsigned)(plane * sizeof(float));
    const float4 go = *reinterpret_cast<const float4*>(gO + (size_t)b * plane + pix);
    // (polled and bumped with LDS instructions proper, as in the forward kernels: a poll through a generic pointer is a flat load
    // behind s_waitcnt vmcnt(0) and waits for every tap load and DMA in flight; dynamic LDS starts at address 0)
    typedef volatile __attribute__((address_space(3))) int lds_int;
    constexpr unsigned READY = PATCH_BYTES + 4 * TAI_FWD_ROWLOOP_RING_SLOTS * 1024;
    auto ready = []() -> lds_int& { return *reinterpret_cast<lds_int*>(READY); };
    if constexpr (EARLY) {
        if (tid == 0) ready() = 0;
        __syncthreads();                   // at kernel entry: nothing is in flight yet
        if (is_gh) {
            bool edge_valid; unsigned edge_lds;
            const float2 e = fwd::stage_patch_dma<PR, 4>(in + ((size_t)b * Hp) * Wp, Hp, Wp, y0, x0, wave, lane, edge_valid, edge_lds);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (edge_valid) asm volatile("ds_write_b64 %0, %1" : : "v"(edge_lds), "v"(e) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) asm volatile("ds_add_u32 %0, %1" : : "v"(READY), "v"(1) : "memory");
            while (ready() < 4) __builtin_amdgcn_s_sleep(1);
        }
    } else {
        __syncthreads();
    }

    if (is_gh ? gH == nullptr : gV == nullptr) return;       // wave-uniform; no workgroup barrier follows
    if (is_gh) {
        const float* vb = vt + ((size_t)b * KS) * plane;
        const unsigned ring_m0 = PATCH_BYTES + __builtin_amdgcn_readfirstlane(wave) * (TAI_FWD_ROWLOOP_RING_SLOTS * 1024);
        const unsigned ring_addr = ring_m0 + lane * 16;
        fwd::TapRegs acc;
        asm volatile(TAI_FWD_ROWLOOP_B_ASM
                     : "={v[0:31]}"(acc.a0), "={v[32:63]}"(acc.a1), "={v[64:95]}"(acc.a2), "={v[96:127]}"(acc.a3),
                       "={v[128:159]}"(acc.a4), "={v[160:191]}"(acc.a5), "={v[192:203]}"(acc.a6)
                     : "{v240}"(row_addr), "{v241}"(ring_addr), "{v242}"(goff), "{s[60:61]}"(vb), "{s62}"(plane_bytes),
                       "{s63}"(ring_m0)
                     : TAI_FWD_ROWLOOP_B_CLOBBERS);
        if (active) store_scaled_taps<0>(gH + ((size_t)b * KS) * plane + pix, acc, go, plane);
    } else {
        const float* hp = ht + ((size_t)b * KS) * plane + pix;
        float* gvb = gV + ((size_t)b * KS) * plane;
        fwd::TapRegs taps;
        fwd::load_taps<0>(taps, hp, plane);
        if constexpr (EARLY) {             // (an LDS read: it does not wait for the tap loads in flight)
            while (ready() < 4) __builtin_amdgcn_s_sleep(1);
        }
        const unsigned long long mask = __ballot(active);
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const f32x4 gov = {go.x, go.y, go.z, go.w};
#define TAI_GV_CALL(ASM_TEXT) \
        asm volatile(ASM_TEXT \
                     : \
                     : "{v[0:31]}"(taps.a0), "{v[32:63]}"(taps.a1), "{v[64:95]}"(taps.a2), "{v[96:127]}"(taps.a3), \
                       "{v[128:159]}"(taps.a4), "{v[160:191]}"(taps.a5), "{v[192:203]}"(taps.a6), "{v240}"(row_addr), \
                       "{v242}"(goff), "{v[244:247]}"(gov), "{s[60:61]}"(gvb), "{s62}"(plane_bytes), "{s[72:73]}"(mask) \
                     : TAI_GV_ROWLOOP_CLOBBERS)
        if constexpr (GVP == 1) { TAI_GV_CALL(TAI_GV_ROWLOOP_ASM_P1); } else if constexpr (GVP == 2) { TAI_GV_CALL(TAI_GV_ROWLOOP_ASM_P2); }
        else { TAI_GV_CALL(TAI_GV_ROWLOOP_ASM); }
#undef TAI_GV_CALL
    }
}

// ---- gI: row-scatter through LDS -----------------------------------------------------------------------------------
// gI[c, y+fy, X] += sum_fx a[c, fy][y, X-fx] * h[fx][y, X-fx]      with  a[c, fy][y, x] = gO[c, y, x] * v[fy][y, x]
// In gather form every term needs v and h of a DIFFERENT source pixel (the reference's kernel: 2,601 x 3 uncached-by-
// design loads per output, its slowest kernel).  Here the scatter is split by axis:
//   * along x it is turned into a GATHER with register-resident taps: a wave owns one source row y; lane G owns the
//     four output columns X = 4G..4G+3 of that row (45 lanes cover the 178 padded columns of a 128-wide tile) and keeps
//     the SHEARED taps hs[i][fx] = h[fx][y, X_i - fx] in 204 VGPRs -- built once per tile by bouncing each coalesced
//     16-byte tap load through a wave-private LDS row and reading it back shifted by fx (zeros outside the row);
//   * per tap row fy the 32 source lanes write a = gO * v[fy] to a wave-private LDS row (v streamed 16 bytes per lane,
//     exactly once), every lane reads its 56-value window with aligned ds_read_b128 and forms its four row sums with
//     the same 4-FMAs-per-LDS-value inner product as the forward kernel;
//   * along y the four sums are added to row (y - y0 + fy) of a workgroup LDS accumulation patch (exclusive per wave and
//     step, one barrier per step), and the patch is added to global gI (zeroed by the launcher) with float atomics once
//     at the end: tiles overlap by ks-1 rows.
// Tiles meet in global atomics, so the last bits of gI depend on arrival order (the forward pass and gV / gH are
// bit-reproducible); the bounds are those of any fp32 summation order (tests: 2e-5 relative to the fp64 oracle).
template <int KS, int NC>
__global__ __launch_bounds__(512, 2)
void sepconv_grad_i_rows(const float* __restrict__ gO, const float* __restrict__ vt, const float* __restrict__ ht,
                         float* __restrict__ gI, int H, int W, int tiles_x, int tiles_y) {
    constexpr int ROWS = 8;                       // source rows per workgroup = waves
    constexpr int PR = ROWS + KS - 1;             // 58 output rows
    constexpr int PITCH = 180;                    // 128 + 50 output columns, padded to a multiple of 4
    constexpr int PAD = 52;                       // left zero pad of the wave rows (>= KS - 1, multiple of 4)
    constexpr int ROWBUF = 320;                   // floats per wave row buffer (covers index 4*44 + 55)
    constexpr int NQ = (TILE_W + KS - 1 + 3) / 4; // 45 output quads
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* patch = lds;                                      // [NC][PR][PITCH]
    float* rows = lds + NC * PR * PITCH;                     // [8 waves][2][ROWBUF]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = fwd::xcd_contiguous_block_id();
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int x0 = tx * TILE_W, y0 = ty * ROWS;
    const int Hp = H + KS - 1, Wp = W + KS - 1;
    const size_t plane = (size_t)H * W;

    for (int i = tid; i < NC * PR * PITCH + 8 * 2 * ROWBUF; i += 512) lds[i] = 0.f;
    __syncthreads();

    float* tapbuf = rows + (wave * 2 + 0) * ROWBUF;
    float* abuf = rows + (wave * 2 + 1) * ROWBUF;
    const int y = y0 + wave;
    const bool src_lane = lane < 32 && y < H && x0 + 4 * lane < W;
    const int yc = min(y, H - 1), xc = min(x0 + 4 * lane, W - 4);
    const size_t pix = (size_t)yc * W + xc;
    const float* hp = ht + ((size_t)b * KS) * plane + pix;
    const float* vp = vt + ((size_t)b * KS) * plane + pix;
    const int G = min(lane, NQ - 1);              // lanes >= NQ shadow the last quad and never write

    // ---- sheared taps, in place: first every tap plane's 16 bytes per source lane (all 51 loads in flight together, as in
    //      the forward kernel), then each float4 is bounced through the wave's LDS row and read back shifted by fx:
    //      hq[fx].{x,y,z,w} = h[fx][y, X_i - fx] for the lane's four OUTPUT columns X_i (zero outside the source columns).
    float4 hq[KS];
#pragma unroll
    for (int fx = 0; fx < KS; ++fx) {
        hq[fx] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src_lane) hq[fx] = *reinterpret_cast<const float4*>(hp + (size_t)fx * plane);
    }
#pragma unroll
    for (int fx = 0; fx < KS; ++fx) {
        if (lane < 32) *reinterpret_cast<float4*>(tapbuf + PAD + 4 * lane) = hq[fx];
        __builtin_amdgcn_wave_barrier();
        const float* tp = tapbuf + PAD + 4 * G - fx;
        hq[fx] = make_float4(tp[0], tp[1], tp[2], tp[3]);
        __builtin_amdgcn_wave_barrier();
    }
    float4 go[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        go[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src_lane) go[c] = *reinterpret_cast<const float4*>(gO + ((size_t)(b * NC + c)) * plane + pix);
    }

    // v planes: VD rows in flight per lane (the row loop is unrolled by VD so the prefetch registers rotate by name)
    constexpr int VD = 1;
    static_assert(KS % VD == 0, "row loop is unrolled by VD");
    float4 vq[VD];
#pragma unroll
    for (int d = 0; d < VD; ++d)
        vq[d] = src_lane ? *reinterpret_cast<const float4*>(vp + (size_t)d * plane) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int fy0 = 0; fy0 < KS; fy0 += VD) {
#pragma unroll
        for (int d = 0; d < VD; ++d) {
            const int fy = fy0 + d;
            const float4 vv = vq[d];
            if (src_lane) vq[d] = *reinterpret_cast<const float4*>(vp + (size_t)min(fy + VD, KS - 1) * plane);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (lane < 32)
                    *reinterpret_cast<float4*>(abuf + PAD + 4 * lane) =
                        make_float4(go[c].x * vv.x, go[c].y * vv.y, go[c].z * vv.z, go[c].w * vv.w);
                __builtin_amdgcn_wave_barrier();
                // window w[j] = a[4G + j - PAD], j = 0..55;  r_i = sum_fx hq[fx][i] * w[PAD + i - fx]
                const float4* wp = reinterpret_cast<const float4*>(__builtin_assume_aligned(abuf + 4 * G, 16));
                float r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 14; ++k) {
                    const float4 w = wp[k];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = 4 * k + e;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int fx = PAD + i - j;
                            if (fx >= 0 && fx < KS) r[i] = fmaf(comp(hq[fx], i), comp(w, e), r[i]);
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
                // Row (wave + fy) of the patch belongs to THIS wave for the duration of step fy (the eight waves of the
                // workgroup hold eight different rows, and the barrier below keeps them on the same fy): a plain
                // 16-byte read-modify-write.  (ds_add_f32 here cost ~150 LDS cycles per wave-instruction: 25x the
                // forward kernel's whole LDS time.)
                if (lane < NQ) {
                    float4* dst = reinterpret_cast<float4*>(patch + (c * PR + wave + fy) * PITCH + 4 * lane);
                    float4 acc = *dst;
                    acc.x += r[0]; acc.y += r[1]; acc.z += r[2]; acc.w += r[3];
                    *dst = acc;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // ---- flush: patch rows y0..y0+57, columns x0..x0+177 of the padded gradient
    for (int c = 0; c < NC; ++c) {
        float* dstp = gI + ((size_t)(b * NC + c) * Hp) * Wp;
        for (int idx = tid; idx < PR * (TILE_W + KS - 1); idx += 512) {
            const int r = idx / (TILE_W + KS - 1), cc = idx - r * (TILE_W + KS - 1);
            const int gy = y0 + r, gx = x0 + cc;
            if (gy < Hp && gx < Wp) atomicAdd(dstp + (size_t)gy * Wp + gx, patch[(c * PR + r) * PITCH + cc]);
        }
    }
}

// ---- gI, second form: wave-private accumulation strips, no per-step workgroup barrier on the accumulators, no atomics ---
// Same algebra as sepconv_grad_i_rows (the scatter along x turned into a gather with register-resident SHEARED taps), with
// the work laid out so that everything that must be summed inside a tile is summed by ONE wave:
//   * a tile is R = 10 source rows x 128 columns; its gradient patch is (R + 50) rows x 178 columns = 45 output quads;
//   * lane l of wave w owns (source row r = l / 6, output quad q = 6 w + l % 6): a wave owns a 6-quad column strip of the
//     patch for ALL source rows of the tile (60 of 64 lanes busy, 45 of 48 strips quads real: 88 % of the lanes do work, the
//     first form's one-row-per-wave layout gave 70 %).  Contributions to output row r + fy from different source rows r
//     therefore meet inside one wave, in program order, in a wave-private LDS accumulator strip ((R + 50) x 6 quads,
//     plain 16-byte read-modify-write, conflict-free): no workgroup barrier orders them and no atomic is needed;
//   * the taps fold gO in: S[fx][i] = (gO h[fx])[y, X_i - fx], so the row loop needs only the v planes, which all waves read
//     from a shared LDS ring that is filled three planes at a time (one barrier per three tap rows, double buffered);
//     row pitch 152 floats makes the 14 window reads of a step conflict-free for this lane layout (verified by
//     enumeration of the ds_read_b128 lane groups);
//   * tiles overlap by 50 rows (and 50 columns when W > 128): each tile writes its patch to a scratch slab and a second
//     small kernel sums the slabs in a fixed order -- bit-reproducible, no memset.  The scratch is the caller's own
//     grad_vertical (or grad_horizontal) buffer, which tai_sepconv_backward fills afterwards; with neither requested the
//     flush falls back to float atomics on a zeroed gI.
// Positions of a window that fall outside the source row hold other rows' (finite) v values or zeros and meet S = 0.
namespace gi2 {
constexpr int KS = 51, R = 10, Q = 6, WAVES = 8, NQ = 45, P = 152, NS = 3, GUARD = 64;
constexpr int PLANE = GUARD + R * P + GUARD;        // floats per staged plane (zero guards front and back)
constexpr int NBUF = 3;                             // stage buffers: the DMA runs two stages ahead of the reads
constexpr int RING = NBUF * NS * PLANE;
constexpr int AROWS = R + KS - 1;                   // 60 accumulator rows per strip
constexpr int ACC = AROWS * Q * 4;                  // floats per wave strip
constexpr int LDS_FLOATS = RING + WAVES * ACC;
constexpr int SPITCH = 180;                         // scratch slab row pitch (floats)
constexpr int SLAB = AROWS * SPITCH;
typedef float vf4 __attribute__((ext_vector_type(4)));
}  // namespace gi2

template <int NC>
__global__ __launch_bounds__(512, 2)
void sepconv_grad_i_strips(const float* __restrict__ gO, const float* __restrict__ vt, const float* __restrict__ ht,
                           float* __restrict__ dst, int H, int W, int tiles_x, int tiles_y, int to_scratch) {
    using namespace gi2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ring = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* acc = lds + RING + wave * ACC;

    int bid = fwd::xcd_contiguous_block_id();
    const int tile = bid;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int x0 = tx * TILE_W, y0 = ty * R;
    const int Hp = H + KS - 1, Wp = W + KS - 1;
    const size_t plane = (size_t)H * W;

    // consumer role: (source row r, output quad q); lanes 60-63 shadow row R-1 and never write
    const int r = min(lane / Q, R - 1), j = lane % Q, q = wave * Q + j;
    const bool owner = lane < R * Q;
    // staging role: thread t < 320 owns 4 source pixels of row sr
    const int sr = tid >> 5, sq = tid & 31;
    const bool stager = tid < R * 32;
    const int sy = y0 + sr, sx = x0 + 4 * sq;
    const bool svalid = stager && sy < H && sx < W;
    const size_t spix = (size_t)min(sy, H - 1) * W + min(sx, W - 4);
    const int soff = GUARD + sr * P + 4 * sq;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int i = tid; i < RING; i += 512) ring[i] = 0.f;          // guards and row gaps stay zero (finite) for good
    const float* win0 = ring + GUARD + r * P + 4 * q - 52;         // window of the lane's row, plane 0 of stage buffer 0

#pragma unroll 1
    for (int c = 0; c < NC; ++c) {
        for (int i = lane; i < ACC; i += 64) acc[i] = 0.f;
        __syncthreads();
        // ---- sheared taps S[fx] = (gO h[fx])[y, X_i - fx], three planes per barrier through the ring
        const float4 go = svalid ? *reinterpret_cast<const float4*>(gO + ((size_t)(b * NC + c)) * plane + spix) : zero4;
        const float* hp = ht + ((size_t)b * KS) * plane + spix;
        float4 S[KS];
        float4 st[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) st[k] = svalid ? *reinterpret_cast<const float4*>(hp + (size_t)k * plane) : zero4;
#pragma unroll
        for (int s = 0; s < KS / NS; ++s) {
            float* buf = ring + (s & 1) * NS * PLANE;
            if (stager) {
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    *reinterpret_cast<float4*>(buf + k * PLANE + soff) =
                        make_float4(go.x * st[k].x, go.y * st[k].y, go.z * st[k].z, go.w * st[k].w);
            }
            if (s + 1 < KS / NS) {
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    st[k] = svalid ? *reinterpret_cast<const float4*>(hp + (size_t)((s + 1) * NS + k) * plane) : zero4;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int fx = s * NS + k;
                const float* row = buf + k * PLANE + GUARD + r * P;
                float t[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int x = 4 * q + i - fx;                  // source column inside the tile
                    const float val = row[max(min(x, TILE_W - 1), 0)];
                    t[i] = (x >= 0 && x < TILE_W) ? val : 0.f;     // (invalid source pixels were staged as zeros)
                }
                S[fx] = make_float4(t[0], t[1], t[2], t[3]);
            }
        }
        __syncthreads();     // every wave is done with the tap planes before v planes overwrite the ring

        // ---- row loop: v planes through the same ring, three tap rows per barrier.  The planes arrive by LDS-DMA
        // (global_load_lds_dwordx4: no staging registers -- the 204 tap registers leave none): wave w copies source rows w
        // and w + 8 of each plane, 32 lanes x 16 bytes per row, one stage ahead of its use.
        auto dma_stage = [&](int s2) {
            const int boff2 = (s2 % NBUF) * NS * PLANE;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const int row = wave + 8 * rr;                               // wave-uniform
                    if (row < R && y0 + row < H) {
                        const unsigned long long src = reinterpret_cast<unsigned long long>(
                            vt + ((size_t)b * KS + (size_t)(s2 * NS + k)) * plane + (size_t)(y0 + row) * W + x0);
                        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)src);
                        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(src >> 32));
                        const float* sp = reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
                        const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)((boff2 + k * PLANE + GUARD + row * P) * 4));
                        if (lane < 32 && x0 + 4 * lane < W)
                            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                                         : : "s"(m0v), "v"(lane * 16), "s"(sp) : "memory");
                    }
                }
            }
        };
        // DMA instructions this wave issues per stage (rows w and w + 8 that exist in the image): the counted wait below
        // leaves exactly the newest stage in flight
        const int my_rows = (y0 + wave < H ? 1 : 0) + (wave + 8 < R && y0 + wave + 8 < H ? 1 : 0);
        dma_stage(0);
        dma_stage(1);
#pragma unroll 1
        for (int s = 0; s < KS / NS; ++s) {
            const int boff = (s % NBUF) * NS * PLANE;
            // this wave's rows of stage s have landed (stage s + 1 may still be in flight: HBM latency under load is longer
            // than the three tap rows a stage lasts)
            if (s + 1 >= KS / NS || my_rows == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (my_rows == 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            __syncthreads();                                        // ... everyone's have, and stage s-1 is consumed
            if (s + 2 < KS / NS) dma_stage(s + 2);
#pragma unroll 1
            for (int k = 0; k < NS; ++k) {
                // (a clang vector type keeps each window chunk ONE 16-byte load = ds_read_b128; through HIP's float4 struct
                // the chunks came out as ds_read2_b64, twice the LDS cycles)
                const vf4* wp = reinterpret_cast<const vf4*>(__builtin_assume_aligned(win0 + boff + k * PLANE, 16));
                float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int m = 0; m < 14; ++m) {
                    const vf4 w = wp[m];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int jj = 4 * m + e;                  // window index: v column 4q - 52 + jj
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int fx = 52 + i - jj;
                            if (fx >= 0 && fx < KS) o[i] = fmaf(comp(S[fx], i), w[e], o[i]);
                        }
                    }
                }
                if (owner) {
                    vf4* a = reinterpret_cast<vf4*>(__builtin_assume_aligned(acc + ((r + s * NS + k) * Q + j) * 4, 16));
                    vf4 t = *a;
                    t[0] += o[0]; t[1] += o[1]; t[2] += o[2]; t[3] += o[3];
                    *a = t;
                }
            }
        }
        __syncthreads();     // (the next channel's tap planes reuse the ring)

        // ---- flush the wave's strip: rows y0 .. y0+59, columns x0 + 24 w .. x0 + 24 w + 23 of the padded gradient
        if (to_scratch) {
            float* slab = dst + ((size_t)tile * NC + c) * SLAB;
            for (int idx = lane; idx < AROWS * Q; idx += 64) {
                const int row = idx / Q, jq = idx - row * Q, qq = wave * Q + jq;
                if (qq < NQ) *reinterpret_cast<float4*>(slab + row * SPITCH + 4 * qq) = *reinterpret_cast<const float4*>(acc + idx * 4);
            }
        } else {
            float* gi = dst + ((size_t)(b * NC + c) * Hp) * Wp;
            for (int idx = lane; idx < AROWS * Q * 4; idx += 64) {
                const int row = idx / (Q * 4), col = idx - row * (Q * 4);
                const int gy = y0 + row, gx = x0 + wave * Q * 4 + col;
                if (gy < Hp && gx < Wp && wave * Q * 4 + col < TILE_W + KS - 1) atomicAdd(gi + (size_t)gy * Wp + gx, acc[idx]);
            }
        }
    }
}

// ---- the strips kernel with its row loop in generated assembly (tools/gen_fwd_asm.py, gen_gi) -----------------------------
// Same tiling, ring, strips and slabs as sepconv_grad_i_strips; what changes is the row loop: the sheared taps sit in the
// forward kernel's register order (v[51 p + t] = S'_p[t] = (gO h[50 - t])[y, X_p - (50 - t)]) with the lane's four output
// columns moved two to the left (X_p = 4q - 2 + p), which makes a tap row exactly the forward's inner product over a
// 16-byte-aligned 54-value window of the v row: 100 v_pk_fma_f32 + 4 v_fmac_f32 instead of 204 scalar FMAs, window reads
// three chunks ahead behind counted lgkmcnt, the accumulator row fetched at the start of the step, the DMA and the stage
// barrier issued from inside the loop.  A strip therefore holds columns X + 2 (the slab sum and the atomic flush shift back).
template <int FX>
__device__ __forceinline__ void gi_tap_plane(fwd::TapRegs& taps, const float* row, int q) {
    // S'_i[50 - FX] = (gO h[FX])[y, x],  x = 4q - 2 + i - FX inside the tile, else 0
#define TAI_GI_TAP(i)                                                                     \
    {                                                                                     \
        const int x = 4 * q - 2 + i - FX;                                                 \
        const float val = row[max(min(x, TILE_W - 1), 0)];                                \
        fwd::tap_set<51 * i + 50 - FX>(taps, (x >= 0 && x < TILE_W) ? val : 0.f);         \
    }
    TAI_GI_TAP(0) TAI_GI_TAP(1) TAI_GI_TAP(2) TAI_GI_TAP(3)
#undef TAI_GI_TAP
}

template <int S>
__device__ __forceinline__ void gi_tap_stages(fwd::TapRegs& taps, float* ring, const float* hp, size_t plane, const float4& go,
                                              bool stager, bool svalid, int soff, int r, int q, float4* st) {
    using namespace gi2;
    if constexpr (S < KS / NS) {
        float* buf = ring + (S & 1) * NS * PLANE;
        if (stager) {
#pragma unroll
            for (int k = 0; k < NS; ++k)
                *reinterpret_cast<float4*>(buf + k * PLANE + soff) = make_float4(go.x * st[k].x, go.y * st[k].y, go.z * st[k].z, go.w * st[k].w);
        }
        if constexpr (S + 1 < KS / NS) {
#pragma unroll
            for (int k = 0; k < NS; ++k)
                st[k] = svalid ? *reinterpret_cast<const float4*>(hp + (size_t)((S + 1) * NS + k) * plane) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        gi_tap_plane<S * NS + 0>(taps, buf + 0 * PLANE + GUARD + r * P, q);
        gi_tap_plane<S * NS + 1>(taps, buf + 1 * PLANE + GUARD + r * P, q);
        gi_tap_plane<S * NS + 2>(taps, buf + 2 * PLANE + GUARD + r * P, q);
        gi_tap_stages<S + 1>(taps, ring, hp, plane, go, stager, svalid, soff, r, q, st);
    }
}

template <int NC>
__global__ __launch_bounds__(512, 2)
void sepconv_grad_i_strips_asm(const float* __restrict__ gO, const float* __restrict__ vt, const float* __restrict__ ht,
                               float* __restrict__ dst, int H, int W, int tiles_x, int tiles_y, int to_scratch) {
    using namespace gi2;
    static_assert(NBUF * NS == 9 && PLANE * 4 == 6592, "tools/gen_fwd_asm.py (GI_SLOTS, GI_PLANE_BYTES) assumes this ring");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ring = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* acc = lds + RING + wave * ACC;

    int bid = fwd::xcd_contiguous_block_id();
    const int tile = bid;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int x0 = tx * TILE_W, y0 = ty * R;
    const int Hp = H + KS - 1, Wp = W + KS - 1;
    const size_t plane = (size_t)H * W;

    const int r = min(lane / Q, R - 1), j = lane % Q, q = wave * Q + j;
    const int sr = tid >> 5, sq = tid & 31;
    const bool stager = tid < R * 32;
    const int sy = y0 + sr, sx = x0 + 4 * sq;
    const bool svalid = stager && sy < H && sx < W;
    const size_t spix = (size_t)min(sy, H - 1) * W + min(sx, W - 4);
    const int soff = GUARD + sr * P + 4 * sq;

    for (int i = tid; i < RING; i += 512) ring[i] = 0.f;          // guards, row gaps and rows past the image stay zero for good
    // asm operands (dynamic LDS starts at LDS address 0)
    const unsigned win_addr = (unsigned)((GUARD + r * P + 4 * q - 52) * 4);
    const unsigned acc_addr = (unsigned)((RING + wave * ACC + (r * Q + j) * 4) * 4);
    const unsigned lane16 = lane * 16;
    // scalar operands of the asm block, made formally wave-uniform (they are: block and wave indices only)
    auto uni = [](unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
    auto uni_ptr = [&](const float* ptr) {
        const unsigned long long a = reinterpret_cast<unsigned long long>(ptr);
        return reinterpret_cast<const float*>(((unsigned long long)uni((unsigned)(a >> 32)) << 32) | uni((unsigned)a));
    };
    auto uni_mask = [&](unsigned long long m) { return ((unsigned long long)uni((unsigned)(m >> 32)) << 32) | uni((unsigned)m); };
    const unsigned plane_bytes = uni((unsigned)(plane * sizeof(float)));
    const bool row1 = y0 + wave < H;
    const float* src1 = uni_ptr(vt + ((size_t)b * KS) * plane + (size_t)min(y0 + wave, H - 1) * W + x0);
    // ring row w + 8 exists for waves 0 and 1 while it is inside the image: a null source pointer tells the loop to skip it
    // (integer arithmetic: a bool select lives in a lane mask and cannot be handed to the asm block in an SGPR)
    const unsigned long long has2 = (unsigned long long)min(max(min(R - 8 - wave, H - (y0 + wave + 8)), 0), 1);
    const float* src2 = uni_ptr(reinterpret_cast<const float*>(
        reinterpret_cast<unsigned long long>(vt + ((size_t)b * KS) * plane + (size_t)min(y0 + wave + 8, H - 1) * W + x0) * has2));
    const unsigned ring1 = uni((unsigned)((GUARD + wave * P) * 4)), ring2 = uni((unsigned)((GUARD + (wave + 8) * P) * 4));
    const unsigned long long dma_mask = uni_mask(__ballot(lane < 32 && x0 + 4 * lane < W && row1));
    const unsigned long long owner_mask = uni_mask(__ballot(lane < R * Q));

#pragma unroll 1
    for (int c = 0; c < NC; ++c) {
        for (int i = lane; i < ACC; i += 64) acc[i] = 0.f;
        __syncthreads();
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 go = svalid ? *reinterpret_cast<const float4*>(gO + ((size_t)(b * NC + c)) * plane + spix) : zero4;
        const float* hp = ht + ((size_t)b * KS) * plane + spix;
        fwd::TapRegs taps;
        float4 st[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) st[k] = svalid ? *reinterpret_cast<const float4*>(hp + (size_t)k * plane) : zero4;
        gi_tap_stages<0>(taps, ring, hp, plane, go, stager, svalid, soff, r, q, st);
        __syncthreads();     // every wave is done with the tap planes before v planes overwrite the ring

        asm volatile(TAI_GI_ROWLOOP_ASM
                     :
                     : "{v[0:31]}"(taps.a0), "{v[32:63]}"(taps.a1), "{v[64:95]}"(taps.a2), "{v[96:127]}"(taps.a3),
                       "{v[128:159]}"(taps.a4), "{v[160:191]}"(taps.a5), "{v[192:203]}"(taps.a6), "{v240}"(win_addr),
                       "{v241}"(acc_addr), "{v242}"(lane16), "{s[60:61]}"(src1), "{s62}"(plane_bytes), "{s63}"(ring1),
                       "{s[72:73]}"(dma_mask), "{s[74:75]}"(owner_mask), "{s77}"(ring2), "{s[78:79]}"(src2)
                     : TAI_GI_ROWLOOP_CLOBBERS);
        __syncthreads();     // (the next channel's tap planes reuse the ring)

        // ---- flush the wave's strip: strip column 4 qq + p holds gradient column x0 + 4 qq + p - 2
        if (to_scratch) {
            float* slab = dst + ((size_t)tile * NC + c) * SLAB;
            for (int idx = lane; idx < AROWS * Q; idx += 64) {
                const int row = idx / Q, jq = idx - row * Q, qq = wave * Q + jq;
                if (qq < NQ) *reinterpret_cast<float4*>(slab + row * SPITCH + 4 * qq) = *reinterpret_cast<const float4*>(acc + idx * 4);
            }
        } else {
            float* gi = dst + ((size_t)(b * NC + c) * Hp) * Wp;
            for (int idx = lane; idx < AROWS * Q * 4; idx += 64) {
                const int row = idx / (Q * 4), col = idx - row * (Q * 4);
                const int gy = y0 + row, tc = wave * Q * 4 + col - 2, gx = x0 + tc;
                if (gy < Hp && gx < Wp && tc >= 0 && tc < TILE_W + KS - 1) atomicAdd(gi + (size_t)gy * Wp + gx, acc[idx]);
            }
        }
    }
}

// gI[b,c,Y,X] = sum of the tile slabs that cover (Y, X), in tile order (fixed: bit-reproducible).  One thread per two columns.
__global__ __launch_bounds__(256)
void sepconv_grad_i_reduce(const float* __restrict__ slabs, float* __restrict__ gI, int n, int NC, int H, int W, int tiles_x,
                           int tiles_y, int xshift) {
    using namespace gi2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int Hp = H + KS - 1, Wp = W + KS - 1, W2 = Wp / 2;
    const int X = 2 * (idx % W2), Y = (idx / W2) % Hp, bc = idx / (W2 * Hp);
    const int b = bc / NC, c = bc - b * NC;
    const int ty_lo = max(0, (Y - (AROWS - 1) + R - 1) / R), ty_hi = min(tiles_y - 1, Y / R);
    const int tx_lo = max(0, (X - (TILE_W + KS - 2) + TILE_W - 1) / TILE_W), tx_hi = min(tiles_x - 1, X / TILE_W);
    float2 s = make_float2(0.f, 0.f);
    for (int ty = ty_lo; ty <= ty_hi; ++ty)
        for (int tx = tx_lo; tx <= tx_hi; ++tx) {
            const size_t tile = ((size_t)b * tiles_y + ty) * tiles_x + tx;
            // (xshift: the assembly strips hold gradient column X at strip column X + 2)
            const float2 p = *reinterpret_cast<const float2*>(slabs + (tile * NC + c) * SLAB + (Y - ty * R) * SPITCH + (X - tx * TILE_W) + xshift);
            s.x += p.x; s.y += p.y;
        }
    *reinterpret_cast<float2*>(gI + ((size_t)bc * Hp + Y) * Wp + X) = s;
}

// ---- generic (any shape / ks / C) versions: one thread per gradient element.
__global__ __launch_bounds__(256)
void sepconv_grad_v_generic(const float* __restrict__ gO, const float* __restrict__ in,
                            const float* __restrict__ ht, float* __restrict__ gV, int n, int C, int H,
                            int W, int ks) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int x = idx % W, y = (idx / W) % H, fy = (idx / (W * H)) % ks, b = idx / (W * H * ks);
    const int Hp = H + ks - 1, Wp = W + ks - 1;
    const size_t plane = (size_t)H * W;
    const float* hp = ht + (size_t)b * ks * plane + (size_t)y * W + x;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* ip = in + ((size_t)(b * C + c) * Hp + y + fy) * Wp + x;
        float r = 0.f;
        for (int fx = 0; fx < ks; ++fx) r = fmaf(hp[(size_t)fx * plane], ip[fx], r);
        acc = fmaf(gO[((size_t)(b * C + c)) * plane + (size_t)y * W + x], r, acc);
    }
    gV[idx] = acc;
}

__global__ __launch_bounds__(256)
void sepconv_grad_h_generic(const float* __restrict__ gO, const float* __restrict__ in,
                            const float* __restrict__ vt, float* __restrict__ gH, int n, int C, int H,
                            int W, int ks) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int x = idx % W, y = (idx / W) % H, fx = (idx / (W * H)) % ks, b = idx / (W * H * ks);
    const int Hp = H + ks - 1, Wp = W + ks - 1;
    const size_t plane = (size_t)H * W;
    const float* vp = vt + (size_t)b * ks * plane + (size_t)y * W + x;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* ip = in + ((size_t)(b * C + c) * Hp + y) * Wp + x + fx;
        float r = 0.f;
        for (int fy = 0; fy < ks; ++fy) r = fmaf(vp[(size_t)fy * plane], ip[(size_t)fy * Wp], r);
        acc = fmaf(gO[((size_t)(b * C + c)) * plane + (size_t)y * W + x], r, acc);
    }
    gH[idx] = acc;
}

// gI: thread per (b, Y, X) of the padded grid, all channels at once (v*h fetched once per tap).
template <int NC>
__global__ __launch_bounds__(256)
void sepconv_grad_i_gather(const float* __restrict__ gO, const float* __restrict__ vt,
                           const float* __restrict__ ht, float* __restrict__ gI, int n, int C, int c0,
                           int H, int W, int ks) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int Hp = H + ks - 1, Wp = W + ks - 1;
    const int X = idx % Wp, Y = (idx / Wp) % Hp, b = idx / (Wp * Hp);
    const size_t plane = (size_t)H * W;
    const float* vb = vt + (size_t)b * ks * plane;
    const float* hb = ht + (size_t)b * ks * plane;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    const int fy_lo = max(0, Y - (H - 1)), fy_hi = min(ks - 1, Y);
    const int fx_lo = max(0, X - (W - 1)), fx_hi = min(ks - 1, X);
    for (int fy = fy_lo; fy <= fy_hi; ++fy) {
        const int y = Y - fy;
        for (int fx = fx_lo; fx <= fx_hi; ++fx) {
            const int x = X - fx;
            const size_t pix = (size_t)y * W + x;
            const float vh = vb[(size_t)fy * plane + pix] * hb[(size_t)fx * plane + pix];
#pragma unroll
            for (int c = 0; c < NC; ++c)
                acc[c] = fmaf(gO[((size_t)(b * C + c0 + c)) * plane + pix], vh, acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) gI[((size_t)(b * C + c0 + c) * Hp + Y) * Wp + X] = acc[c];
}

}  // namespace bwd
