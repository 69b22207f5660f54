// 3x3 stride-1 "same" convolution, fp32, as Winograd F(4x4, 3x3) on the fp32 MFMA pipe (included by sepconv_capi.hip).
//
// F(2x2, 3x3) -- wino_conv.hip.inc -- spends 16 multiplies on a 2 x 2 output tile, F(4x4, 3x3) spends 36 on a 4 x 4 tile: 1.78x fewer MFMAs
// for the same layer,
//     Y = A^T [ (G g G^T) .* (B^T d B) ] A          d: 6x6 input patch, g: 3x3 filter, Y: 4x4 outputs
// on the interpolation points (0, +-3/4, +-3/2, inf) (round 5: a quarter of the fp32 rounding of Lavin's 0, +-1, +-2, inf; below).  It
// replaces the same reference layers as wino_conv.hip.inc (src/models/mcnet/mcnet.py:79-118,131-152,165-176,198-224;
// src/models/tai/tai.py:248-286) and, read as displaced 3 x 3 blocks, MotionEnc's 5 x 5 / 7 x 7 layers (mcnet.py:36-47); conv_ops decides
// which layers take it (conv_ops._wino43_ok, set_winograd_tile).
//
// Work decomposition (one workgroup = 8 waves = one CU, two waves per SIMD; the chunk loop is generated: tools/gen_wino43_asm.py):
//   * a workgroup owns 64 output channels x 32 tiles (4x4 output pixels each; tiles numbered (image, ty, tx), tx fastest);
//   * wave (wm 0..3, wn 0..1) owns channels 16 wm .. +15 and tiles 16 wn .. +15 for ALL 36 transform positions on
//     v_mfma_f32_16x16x4_f32 (M = output channels, N = tiles, K = 4 input channels): 36 positions x 4 registers = 144 accumulator
//     registers a[0:143]; a lane holds, for one tile, 4 channels x 36 positions, so the inverse transform is per-lane;
//   * the reduction over input channels runs in chunks of 4 (one MFMA k-step): 36 positions x 64 channels x 4 of transformed weights
//     are 36 KB per chunk -- at 8 input channels two stages would not fit the CU's 160 KB of LDS -- plus 18 KB of transformed patches;
//     LDS is double-buffered (2 x 54 KB), one barrier per chunk;
//   * LDS operand order [position group of 4][k][row][4 positions]: one ds_read_b128 is a lane's A (or B) operand of four positions;
//   * waves 0-3 load and transform the patches -- thread t: patch (tile t % 32, input channel (t / 32) % 4), half t / 128 (wave-uniform):
//     columns 3h .. 3h+2 of B^T d B -- waves 4-7 copy the weights global -> LDS (global_load_lds_dwordx4).
//
// v_mfma_f32_16x16x4_f32 operand map (wave64): A[m][k]: lane = 16 k + m;  B[k][n]: lane = 16 k + n;
// D[m][n]: lane = 16 (m / 4) + n, register = m % 4.

namespace wino43 {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int KC = 4;                          // input channels per chunk
constexpr int TM = 64, TN = 32;                // output channels x tiles per workgroup
constexpr int U_STAGE = 9 * KC * TM * 4;       // floats: [9 position groups][4 k][64 channels][4 positions]
constexpr int V_STAGE = 9 * KC * TN * 4;       // floats: [9][4 k][32 tiles][4 positions]
constexpr int STAGE_FLOATS = U_STAGE + V_STAGE;
constexpr int LDS_BYTES = 2 * STAGE_FLOATS * 4;   // 110,592

// Numbering of the 36 transform positions (row i, column j of the 6 x 6 domain): rows in pairs, the two rows of a pair adjacent --
// a thread that owns three columns of B^T d B then holds, per row pair, six consecutive positions = three 8-byte LDS writes, and one
// ds_read_b128 is still a lane's operand of four positions.
__host__ __device__ constexpr int position(int i, int j) { return ((i >> 1) * 6 + j) * 2 + (i & 1); }

// Interpolation points (0, +-a, +-b, inf) with a = 3/4, b = 3/2 (round 5; Lavin's 0, +-1, +-2, inf until then): the same construction, the same
// transform structure, a quarter of the fp32 rounding error per layer -- tools/wino_f43_points_study.py, tools/gen_wino43_asm.py (A_PT, B_PT:
// the generated B^T and A^T use the same points; every constant there is a multiple of 1/64).  G[point][tap] = point^tap / prod(point - others).
constexpr double PT_A = 0.75, PT_B = 1.5;

// U[kb][chunk][pg][k][ch][j] = (G g G^T)[position 4 pg + j] of output channel 64 kb + ch, input channel 4 chunk + k; zero padded.
__global__ void transform_weights(const float* __restrict__ w, float* __restrict__ U, int K, int C, int Kpad, int Cpad) {
    const long long total = (long long)Kpad * Cpad;
    constexpr double a = PT_A, b = PT_B, n0 = a * a * b * b, na = 2 * a * a * (a * a - b * b), nb = 2 * b * b * (b * b - a * a);
    const double G[6][3] = {{1 / n0, 0., 0.}, {1 / na, a / na, a * a / na}, {1 / na, -a / na, a * a / na},
                            {1 / nb, b / nb, b * b / nb}, {1 / nb, -b / nb, b * b / nb}, {0., 0., 1.}};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % Kpad), c = (int)(i / Kpad);
        double g[3][3];
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) g[x][y] = (k < K && c < C) ? (double)w[((long long)k * C + c) * 9 + x * 3 + y] : 0.0;
        // (in double, rounded once: the weights are transformed once per weight, not per launch)
        double t[6][3];
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) t[x][y] = G[x][0] * g[0][y] + G[x][1] * g[1][y] + G[x][2] * g[2][y];
        const int kb = k / TM, ch = k % TM, chunk = c / KC, kk = c % KC;
        float* dst = U + ((long long)kb * (Cpad / KC) + chunk) * U_STAGE;
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int y = 0; y < 6; ++y) {
                const double u = t[x][0] * G[y][0] + t[x][1] * G[y][1] + t[x][2] * G[y][2];
                const int p = position(x, y);
                dst[(((p >> 2) * KC + kk) * TM + ch) * 4 + (p & 3)] = (float)u;
            }
    }
}

// ---- bias, activation and stores of one channel's 4 x 4 output tile (and the second outputs); raw[i] = row i of A^T m A
// pool_h > 0: the pooled output goes into a plane of pool_h x pool_w with its origin at (pool_oy, pool_ox) (the halo-carrying input plane of
// the next MotionEnc stage; pool_w and pool_ox even), else a plain [N, K, H/2, W/2] tensor
template <int ACT, int EPI>
__device__ __forceinline__ void finish_tile(const f4v (&raw)[4], int k, int eimg, int ety, int etx, const float* __restrict__ bias,
                                            float* __restrict__ y, int K, int H, int W, float* __restrict__ ypool,
                                            const float* __restrict__ addx, float* __restrict__ y2, int pool_h = 0, int pool_w = 0,
                                            int pool_oy = 0, int pool_ox = 0) {
    const float bv = bias[k];
    const long long chan = (long long)eimg * K + k;
    float* yp = y + (chan * H + 4 * ety) * W + 4 * etx;
    typedef float f2v __attribute__((ext_vector_type(2)));
    f2v ax[2] = {f2v{0.f, 0.f}, f2v{0.f, 0.f}};
    if (EPI == 2 || EPI == 3) {            // the four values that land on the tile's even sites: rows 2 ety, 2 ety + 1 of addx
        const float* ap = addx + (chan * (H >> 1) + 2 * ety) * (W >> 1) + 2 * etx;
        ax[0] = *reinterpret_cast<const f2v*>(ap);
        ax[1] = *reinterpret_cast<const f2v*>(ap + (W >> 1));
    }
    f4v orow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float o0 = raw[i].x + bv, o1 = raw[i].y + bv, o2 = raw[i].z + bv, o3 = raw[i].w + bv;
        if (ACT == 1) { o0 = fmaxf(o0, 0.f); o1 = fmaxf(o1, 0.f); o2 = fmaxf(o2, 0.f); o3 = fmaxf(o3, 0.f); }
        if (ACT == 2) { o0 = tanhf(o0); o1 = tanhf(o1); o2 = tanhf(o2); o3 = tanhf(o3); }
        orow[i] = f4v{o0, o1, o2, o3};
        if (EPI != 3) *reinterpret_cast<f4v*>(yp + (long long)i * W) = orow[i];
        if (EPI == 2 || EPI == 3) {
            f4v sum = orow[i];
            if ((i & 1) == 0) { sum.x += ax[i >> 1].x; sum.z += ax[i >> 1].y; }
            float* dst = (EPI == 2 ? y2 : y) + (chan * H + 4 * ety + i) * W + 4 * etx;
            *reinterpret_cast<f4v*>(dst) = sum;
        }
    }
    if (EPI == 1) {
        const int ph = pool_h > 0 ? pool_h : (H >> 1), pw = pool_h > 0 ? pool_w : (W >> 1);
        float* pp = ypool + (chan * ph + (pool_h > 0 ? pool_oy : 0) + 2 * ety) * pw + (pool_h > 0 ? pool_ox : 0) + 2 * etx;
        *reinterpret_cast<f2v*>(pp) = f2v{fmaxf(fmaxf(orow[0].x, orow[0].y), fmaxf(orow[1].x, orow[1].y)),
                                          fmaxf(fmaxf(orow[0].z, orow[0].w), fmaxf(orow[1].z, orow[1].w))};
        *reinterpret_cast<f2v*>(pp + pw) = f2v{fmaxf(fmaxf(orow[2].x, orow[2].y), fmaxf(orow[3].x, orow[3].y)),
                                               fmaxf(fmaxf(orow[2].z, orow[2].w), fmaxf(orow[3].z, orow[3].w))};
    }
}

// ---- The kernel: the whole channel-chunk loop is ONE generated asm statement (tools/gen_wino43_asm.py -> wino43_chunkloop.inc; round 5;
// round 4's compiler-scheduled four- and eight-wave forms are in the history: DESIGN.md 4.4c): eight waves, 16 channels x 16 tiles x 36 positions = 144 accumulators a[0:143] each;
// waves 0-1 load and transform columns 0-2 of the patches, waves 2-3 columns 3-5, waves 4-7 copy the weights; every load, wait, LDS
// address and MFMA has a fixed register and place, so nothing depends on how the compiler allocates or schedules around asm loads
// (ADVICE r04: the compiler-scheduled form's edge loads were only safe while no spill or copy touched their registers).  This function
// computes the loop's inputs (per-lane byte offsets of the six patch rows, LDS bases, the parts' base addresses) and runs the
// epilogue on the accumulators the statement returns.
#include "wino43_chunkloop.inc"
#if defined(TAI_W43_WRW_ABLATED) && !defined(TAI_ALLOW_ABLATED)
#error "wino43_chunkloop.inc was generated with TAI_WRW_ABLATE (a timing experiment with wrong results): run tools/gen_wino43_asm.py without it"
#endif
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x16 __attribute__((ext_vector_type(16)));

// BLOCKS (the displaced-read form, tai_conv3x3_wino43_forward_blocks): x is ONE plane [N, cpart, in_h, in_w] that carries its halo, with the
// pixel under output (0, 0)'s centre tap of block (0, 0) at (in_oy, in_ox); C = S * S * cpart channels, channel block (a, b) = block
// a * S + b reads the plane displaced by (3a, 3b) pixels: a k x k "same" convolution (k = 5, 7: MotionEnc, mcnet.py:36-47) with its
// filter cut into S x S blocks of 3 x 3 taps, zero past k.  No bounds tests: the halo covers every read.
struct Window { int in_h, in_w, in_oy, in_ox, S, pool_h, pool_w, pool_oy, pool_ox, zero_taps, dispatch_order, splits, chunks_per_split; };   // zero_taps: 3 S > k (the last blocks carry zero taps); dispatch_order: A/B switch of the workgroup placement below; splits, chunks_per_split: SPLITC below

// SPLITC (split over input channels, small grids; tai_conv3x3_wino43_forward_ws): workgroup (split sp, tile block, channel block) runs the
// same chunk loop over chunks sp * chunks_per_split ... (+ chunks_per_split, the last split fewer) and writes its un-biased 4 x 4 output
// tiles, after the inverse transform, to y = the workspace [splits][N][K][H][W]; splitc_reduce sums them in split order and runs the
// epilogue.  The host breaks splits on part boundaries (a split lies inside one part or covers whole parts), so the loop's per-part state
// only starts at another part and a byte offset.  The other instantiations (SPLITC false) compile to the instruction stream they had.

template <int ACT, int EPI = 0, int VAR = 0, bool BLOCKS = false, bool SPLITC = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv3x3_gen(const float* __restrict__ x, const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ x3,
                 int cpart, const float* __restrict__ U, const float* __restrict__ bias, float* __restrict__ y, int N,
                 int C, int K, int H, int W, int Kpad, int nchunks, int kblocks, float* __restrict__ ypool, const float* __restrict__ addx,
                 float* __restrict__ y2, Window win) {
    static_assert(TAI_W43_STAGE_BYTES == STAGE_FLOATS * 4, "generator and kernel disagree on the LDS stage");
    static_assert(!(SPLITC && (BLOCKS || EPI != 0 || ACT != 0)), "the split form writes raw partial tiles of the plain form");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 3, wn = wave >> 2, ch0 = wm * 16;
    // Workgroup -> (tile block tb, channel block kb).  The hardware deals consecutive workgroups to the 8 XCDs in turn (blockIdx % 8), each with
    // its own L2: an XCD gets ONE channel block where 8 / kblocks is whole (its 36-position weights, 2.4 MB at 256 x 64 channels, then
    // stay in that L2) and a CONTIGUOUS run of tile blocks (neighbouring tile rows share two of their six patch rows, and the run walks the
    // input like a stream); with 8, 16 ... channel blocks an XCD takes kblocks / 8 of them for every tile block.  Any placement gives the
    // same results (round 5; until then tb = blockIdx / kblocks, kb = blockIdx % kblocks).
    int tb, kb, sp = 0;
    {
        int bid = blockIdx.x, nblk = gridDim.x;
        if constexpr (SPLITC) {
            // the splits of one (tile block, channel block) are consecutive workgroups of one XCD: the placement below then runs on the
            // unsplit grid, the XCD's slot divided by the split count
            nblk /= win.splits;
            if (!win.dispatch_order && nblk % 8 == 0) {
                const int s = bid >> 3;
                sp = s % win.splits;
                bid = (s / win.splits) * 8 + (bid & 7);
            } else {
                sp = bid % win.splits;
                bid /= win.splits;
            }
        }
        const int tblocks = nblk / kblocks, xcd = bid & 7, slot = bid >> 3;
        if (win.dispatch_order) {           // tai_conv3x3_wino43_set_placement(0): the placement of rounds 4-5 (A/B timing)
            tb = bid / kblocks;
            kb = bid - tb * kblocks;
        } else if (nblk % 8 == 0 && kblocks <= 8 && 8 % kblocks == 0 && tblocks % (8 / kblocks) == 0) {
            kb = xcd % kblocks;
            tb = (xcd / kblocks) * (tblocks / (8 / kblocks)) + slot;
        } else if (nblk % 8 == 0 && kblocks % 8 == 0) {
            const int per = kblocks / 8;
            kb = xcd * per + slot % per;
            tb = slot / per;
        } else {
            tb = bid / kblocks;
            kb = bid - tb * kblocks;
        }
    }
    const int TH = H >> 2, TW = W >> 2;
    const int tiles_per_image = TH * TW, tiles_total = N * tiles_per_image;
    const long long plane = BLOCKS ? (long long)win.in_h * win.in_w : (long long)H * W;
    u32x16 vin;
    {
        // patch role (waves 0-3; the weight-copy waves carry the values unused): tile pl, input channel pk of the chunk, half ph
        const int pl = tid & 31, pk = (tid >> 5) & 3, ph = (tid >> 7) & 1;
        const int pt = tb * TN + pl;
        const bool pvalid = pt < tiles_total;
        const int ptc = pvalid ? pt : 0;
        const int pimg = ptc / tiles_per_image, prem = ptc - pimg * tiles_per_image;
        const int pty = prem / TW, ptx = prem - pty * TW;
        constexpr unsigned OUT_OF_RANGE = 0x80000000u;      // beyond num_records: the buffer load returns 0 (the zero padding)
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            if constexpr (BLOCKS) {
                // column 0 of the patch row in the plane; columns 1-4 follow (one 16-byte load, 4-byte aligned), column 5 after them
                const unsigned base = ((unsigned)(pimg * cpart + pk) * (unsigned)plane +
                                       (unsigned)((win.in_oy - 1 + 4 * pty + r) * win.in_w + win.in_ox - 1 + 4 * ptx)) * 4u;
                vin[r] = pvalid ? base + 4u : OUT_OF_RANGE;
                vin[6 + r] = pvalid ? (ph ? base + 20u : base) : OUT_OF_RANGE;
            } else {
                const int yy = 4 * pty - 1 + r;
                const bool rowok = pvalid && yy >= 0 && yy < H;
                const unsigned base = ((unsigned)(pimg * cpart + pk) * (unsigned)plane + (unsigned)(yy * W + 4 * ptx)) * 4u;
                vin[r] = rowok ? base : OUT_OF_RANGE;
                vin[6 + r] = ph ? ((rowok && ptx < TW - 1) ? base + 16u : OUT_OF_RANGE) : ((rowok && ptx > 0) ? base - 4u : OUT_OF_RANGE);
            }
        }
        const int kq = lane >> 4, l16 = lane & 15;
        vin[12] = (unsigned)((kq * TM + ch0 + l16) * 16);                       // A operand (stage 0, position group 0)
        vin[13] = (unsigned)(U_STAGE * 4 + (kq * TN + wn * 16 + l16) * 16);     // B operand
        vin[14] = (unsigned)(U_STAGE * 4 + (pk * TN + pl) * 16);                // this thread's transformed patch (position group 0)
        vin[15] = (unsigned)(lane * 16);
    }
    typedef int i32x16 __attribute__((ext_vector_type(16)));
    i32x16 sin;
    {
        unsigned long long b[4] = {reinterpret_cast<unsigned long long>(x), reinterpret_cast<unsigned long long>(x1),
                                   reinterpret_cast<unsigned long long>(x2), reinterpret_cast<unsigned long long>(x3)};
        int c0 = 0, nch = nchunks;            // this workgroup's chunks
        long long moved = 0;                  // bytes the (one, ragged) part's base has moved on
        if constexpr (SPLITC) {
            c0 = sp * win.chunks_per_split;
            nch = min(win.chunks_per_split, nchunks - c0);
            // first part p0 at chunk o: the parts from p0 on move into slots 0.. (past the last part: never read), part p0's base moves
            // o chunks on -- the same addresses as the unsplit loop's at chunk c0.  The hardware's range check INCLUDES the scalar offset
            // (a load is out of range when vector offset + scalar offset >= num_records; that is how the unsplit loop, whose chunk offset
            // rides in the scalar offset, gets 0.0 for the last image's channels C .. Cpad - 1) and counts from the base.  So with ONE
            // part of a ragged channel count num_records shrinks by what the base moved: those channels are then past the end exactly
            // as in the unsplit loop (with num_records left whole they were read from behind the tensor's end, up to 3 planes of foreign
            // memory times zero weights).  Only then (cpart == C): several parts are whole chunks each, nothing is read past a part,
            // and their bases are other tensors'.
            const int cpp = (cpart + KC - 1) / KC, p0 = c0 / cpp, o = c0 - p0 * cpp;
            if (cpart == C) moved = (long long)o * KC * plane * 4;
            const unsigned long long q[4] = {b[0], b[1], b[2], b[3]};
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = p0 + i == 1 ? q[1] : p0 + i == 2 ? q[2] : p0 + i == 3 ? q[3] : q[0];
            b[0] += (unsigned long long)o * KC * plane * 4;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sin[2 * i] = __builtin_amdgcn_readfirstlane((int)(unsigned)b[i]);
            sin[2 * i + 1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(b[i] >> 32));
        }
        const unsigned long long ub = reinterpret_cast<unsigned long long>(U) +
            (((unsigned long long)kb * nchunks + c0) * (U_STAGE * 4) + (unsigned long long)(wave & 3) * 1024ull);
        sin[8] = __builtin_amdgcn_readfirstlane((int)((long long)N * cpart * plane * 4 - moved));      // bytes of a part (num_records)
        sin[9] = __builtin_amdgcn_readfirstlane((cpart + KC - 1) / KC);                         // chunks per part (one part: all of them)
        sin[10] = __builtin_amdgcn_readfirstlane(nch);
        sin[11] = __builtin_amdgcn_readfirstlane((int)(KC * plane * 4));                        // bytes from one chunk's channels to the next
        sin[12] = __builtin_amdgcn_readfirstlane((int)(unsigned)ub);
        sin[13] = __builtin_amdgcn_readfirstlane((int)(unsigned)(ub >> 32));
        sin[14] = __builtin_amdgcn_readfirstlane((wave < 2 ? 0 : wave < 4 ? 1 : 2) | ((wave & 3) << 8));
        sin[15] = 0;
        if constexpr (BLOCKS) {      // the slots of parts 1 and 2 carry the block walk: bytes from a row's last block to the next row's first, S
            sin[2] = __builtin_amdgcn_readfirstlane((3 * win.in_w - 3 * (win.S - 1)) * 4);
            sin[4] = __builtin_amdgcn_readfirstlane(win.S);
            sin[6] = __builtin_amdgcn_readfirstlane(win.zero_taps);      // the MFMAs on the last blocks' all-zero transformed rows / columns are skipped
        }
    }
    f32x32 a0, a1, a2, a3;
    f32x16 a4;
#define TAI_W43_LOOP_CALL(ASM_TEXT)                                                                                              \
    asm volatile(ASM_TEXT                                                                                                       \
                 : "={a[0:31]}"(a0), "={a[32:63]}"(a1), "={a[64:95]}"(a2), "={a[96:127]}"(a3), "={a[128:143]}"(a4)               \
                 : "{v[46:61]}"(vin), "{s[48:63]}"(sin)                                                                         \
                 : TAI_W43_LOOP_CLOBBERS)
#ifdef TAI_TIMING_VARIANTS
    if constexpr (VAR == 1) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V1);
    else if constexpr (VAR == 2) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V2);
    else if constexpr (VAR == 3) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V3);
    else if constexpr (VAR == 4) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V4);
    else if constexpr (VAR == 5) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V5);
    else if constexpr (VAR == 6) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V6);
    else if constexpr (VAR == 7) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V7);
    else if constexpr (VAR == 8) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V8);
    else if constexpr (VAR == 9) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V9);
    else if constexpr (VAR == 10) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V10);
    else if constexpr (VAR == 11) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V11);
    else if constexpr (VAR == 12) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_V12);
    else
#endif
    if constexpr (BLOCKS) TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM_BLOCKS);
    else TAI_W43_LOOP_CALL(TAI_W43_LOOP_ASM);
#undef TAI_W43_LOOP_CALL
    // ---- inverse transform per channel register r (generated: the accumulators are read where they lie, a[4 p + r]), then the C++ tail
    const int kq = lane >> 4, l16 = lane & 15;
    const int et = tb * TN + wn * 16 + l16;
    const bool evalid = et < tiles_total;
    const int etc = evalid ? et : 0;
    const int eimg = etc / tiles_per_image, erem = etc - eimg * tiles_per_image;
    const int ety = erem / TW, etx = erem - ety * TW;
#define TAI_W43_INVERSE(R, ASM_TEXT)                                                                                               \
    {                                                                                                                           \
        f32x16 o;                                                                                                               \
        asm volatile(ASM_TEXT : "={v[0:15]}"(o)                                                                                 \
                     : "{a[0:31]}"(a0), "{a[32:63]}"(a1), "{a[64:95]}"(a2), "{a[96:127]}"(a3), "{a[128:143]}"(a4)               \
                     : TAI_W43_INVERSE_CLOBBERS);                                                                               \
        const int k = kb * TM + ch0 + 4 * kq + R;                                                                               \
        if (evalid && k < K) {                                                                                                  \
            const f4v raw[4] = {f4v{o[0], o[1], o[2], o[3]}, f4v{o[4], o[5], o[6], o[7]}, f4v{o[8], o[9], o[10], o[11]},        \
                                f4v{o[12], o[13], o[14], o[15]}};                                                               \
            if constexpr (SPLITC) {                                                                                             \
                float* wp = y + ((((long long)sp * N + eimg) * K + k) * H + 4 * ety) * W + 4 * etx;                             \
                _Pragma("unroll") for (int i = 0; i < 4; ++i) *reinterpret_cast<f4v*>(wp + (long long)i * W) = raw[i];         \
            } else {                                                                                                            \
                finish_tile<ACT, EPI>(raw, k, eimg, ety, etx, bias, y, K, H, W, ypool, addx, y2, win.pool_h, win.pool_w,        \
                                      win.pool_oy, win.pool_ox);                                                                \
            }                                                                                                                   \
        }                                                                                                                       \
    }
    TAI_W43_INVERSE(0, TAI_W43_INVERSE_ASM_R0)
    TAI_W43_INVERSE(1, TAI_W43_INVERSE_ASM_R1)
    TAI_W43_INVERSE(2, TAI_W43_INVERSE_ASM_R2)
    TAI_W43_INVERSE(3, TAI_W43_INVERSE_ASM_R3)
#undef TAI_W43_INVERSE
}

// ---- SPLITC's second step: the partial tiles [splits][N][K][H][W] summed in split order (s = 0, 1, ...: the same bits on every run),
// then finish_tile's bias, activation and second outputs.  One thread per (image, channel, 4 x 4 tile), the tile column fastest.
template <int ACT, int EPI>
__global__ __launch_bounds__(256) void splitc_reduce(const float* __restrict__ ws, int splits, const float* __restrict__ bias,
                                                     float* __restrict__ y, int N, int K, int H, int W, float* __restrict__ ypool,
                                                     const float* __restrict__ addx, float* __restrict__ y2) {
    const int TH = H >> 2, TW = W >> 2;
    const long long total = (long long)N * K * TH * TW, part = (long long)N * K * H * W;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int etx = (int)(t % TW);
        long long r = t / TW;
        const int ety = (int)(r % TH);
        r /= TH;
        const int k = (int)(r % K), eimg = (int)(r / K);
        const float* p = ws + (((long long)eimg * K + k) * H + 4 * ety) * W + 4 * etx;
        f4v raw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) raw[i] = *reinterpret_cast<const f4v*>(p + (long long)i * W);
        for (int s = 1; s < splits; ++s) {
            p += part;
#pragma unroll
            for (int i = 0; i < 4; ++i) raw[i] += *reinterpret_cast<const f4v*>(p + (long long)i * W);
        }
        finish_tile<ACT, EPI>(raw, k, eimg, ety, etx, bias, y, K, H, W, ypool, addx, y2);
    }
}

// ---- Weight gradient in the same transform domain (round 5; tools/gen_wino43_asm.py, "WRW"):
//     dL/dU[pos][k][c] = sum over tiles of (A dY A^T)[pos][k][tile] * (B^T d B)[pos][c][tile],      dL/dg = G^T (dL/dU) G
// -- 36 multiplies per 4 x 4 tile and (k, c) where the F(2x2, 3x3) kernel (wino_wrw.hip.inc) spends 16 per 2 x 2 tile: 1.78x fewer MFMAs.
// The chunk loop is the forward's with the roles renamed: M = 64 output channels, N = 32 INPUT channels, the reduction runs over the tiles,
// four consecutive tiles of a tile row per chunk (W % 16 == 0); a workgroup owns (k block, c block, a contiguous run of chunks = "split")
// and writes G^T m G of its 64 x 32 block to ws[split][tap][Kpad][Cpad], which wino::wrw::wrw_reduce sums in a fixed order (no atomics:
// the gradient is bit-reproducible).  Waves 0-3 transform the input patches (thread = tile tid % 4, channel (tid / 4) % 32, half
// tid / 128), waves 4-7 the output-gradient tiles (lane = tile lane % 4, channel 16 (wave % 4) + lane / 4); the c-block-0 workgroups also sum the output
// gradients they pass (the bias gradient).  Reference: the backward of the same layers (autograd of mcnet.py:79-118,131-152,165-176,198-224).
constexpr int WRW_LDS_BYTES = LDS_BYTES;

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void conv3x3_wrw_gen(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ ws, float* __restrict__ wsb, int N,
                     int C, int K, int H, int W, int kblocks, int cblocks, int Kpad, int Cpad, int chunks_per_split, int nchunks_total,
                     int in_h, int in_w, int in_oy, int in_ox, int dispatch_order) {
    // (in_h, in_w, in_oy, in_ox) = (H, W, 0, 0): an ordinary tensor, zero padding outside.  Otherwise x is a plane of in_h x in_w per channel
    // that carries its own halo, the pixel under output (0, 0) at (in_oy >= 1, in_ox >= 1) (the shifted-copy stack of the 5x5 / 7x7 layers):
    // every row and edge column is read where it lies
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 3, wn = wave >> 2, ch0 = wm * 16;
    // workgroups that the hardware places on one XCD (blockIdx % 8) take consecutive (split, c block, k block) triples: all blocks of a
    // split -- which read the same tiles of x and dy -- then share one L2 (any placement gives the same results)
    const int bid = (gridDim.x % 8 == 0 && !dispatch_order) ? (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
    const int kb = bid % kblocks, cb = (bid / kblocks) % cblocks, sp = bid / (kblocks * cblocks);
    const int TH = H >> 2, CPR = W >> 4;                       // tile rows per image, chunks (of four tiles) per tile row
    const int plane = H * W, plane_in = in_h * in_w;
    const bool halo = in_h != H || in_w != W;
    const int c_first = sp * chunks_per_split;
    const int nch = min(chunks_per_split, nchunks_total - c_first);
    const int n0 = c_first / (TH * CPR), rem0 = c_first - n0 * TH * CPR, ty0 = rem0 / CPR, q0 = rem0 - ty0 * CPR;
    const bool yrole = wave >= 4;
    constexpr unsigned OUT_OF_RANGE = 0x80000000u;
    u32x16 vin;
#pragma unroll
    for (int i = 0; i < 16; ++i) vin[i] = 0;
    // Lanes of a wave are (channel, tile of the chunk) with the TILE fastest: a load instruction then takes 64 contiguous bytes of each of 16
    // planes (with the channel fastest it took 16 bytes of 64 planes -- 64 cache lines per instruction: the CU's address unit, not the
    // matrix pipe, set the pace).  The LDS rows of the four tiles (k-steps) of one channel are 512 / 1024 bytes apart, the same banks: the
    // row index is XORed with swz(tile) = 0, 2, 12, 14.  Writes (ds_write_b128 is served in groups of 8 lanes = 4 tiles x 2 rows, 32 banks):
    // the values are distinct and even modulo 8, so the 8 lanes fall into 8 different 16-byte slots.  Reads (ds_read_b128: groups of 16 lanes
    // made of rows {0-3, 12-15} of one k-step and rows {4-11} of its neighbour): each value has bit 2 == bit 3, which maps both row sets
    // onto themselves -- every aligned group of 16 rows is permuted in itself and an MFMA operand read stays conflict-free.
    auto swz = [](int k) { return (k & 1) * 2 + (k >> 1) * 12; };
    if (!yrole) {
        // patch role: input channel pl of the block, tile pk of the chunk, half ph.  The descriptor's base is x - (W + 1) floats: patch row r
        // of tile row ty is image row 4 ty - 1 + r and the left edge column is pixel 4 tx - 1, so that neither the scalar offset (image,
        // 4 ty, 16 q) nor a lane's offset is ever negative.  Nothing outside the tensor is read: row -1 / H through a zero-size descriptor,
        // the pixel in front of a tile row's first tile / behind its last through EXEC (generator, "WRW")
        const int pk = tid & 3, pl = (tid >> 2) & 31, ph = (tid >> 7) & 1;
        const int c = cb * TN + pl;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const unsigned mid = ((unsigned)c * (unsigned)plane_in + (unsigned)(r * in_w + 4 * pk + 1)) * 4u;
            vin[r] = c < C ? mid : OUT_OF_RANGE;
            vin[6 + r] = c < C ? (ph ? mid + 16u : mid - 4u) : OUT_OF_RANGE;
        }
        vin[14] = (unsigned)(U_STAGE * 4 + (pk * TN + (pl ^ swz(pk))) * 16);
        // the coefficient of the edge value in the lanes whose edge column lies outside the image when the chunk starts / ends a tile row
        const float full = ph ? 1.0f : (float)(PT_A * PT_A * PT_B * PT_B);
        vin[15] = __builtin_bit_cast(unsigned, (!halo && (ph ? pk == 3 : pk == 0)) ? 0.0f : full);
    } else {
        const int t = lane & 3, m = 16 * (wave & 3) + (lane >> 2), k = kb * TM + m;
#pragma unroll
        for (int r = 0; r < 4; ++r) vin[r] = k < K ? ((unsigned)k * (unsigned)plane + (unsigned)(r * W + 4 * t)) * 4u : OUT_OF_RANGE;
        vin[14] = (unsigned)((t * TM + (m ^ swz(t))) * 16);
    }
    {
        const int kq = lane >> 4, l16 = lane & 15;
        vin[12] = (unsigned)((kq * TM + ((ch0 + l16) ^ swz(kq))) * 16);                        // A operand (stage 0, position group 0)
        vin[13] = (unsigned)(U_STAGE * 4 + (kq * TN + ((wn * 16 + l16) ^ swz(kq))) * 16);     // B operand
    }
    typedef int i32x16 __attribute__((ext_vector_type(16)));
    i32x16 sin;
    {
        const int planes = yrole ? K : C;
        const int pl_sz = yrole ? plane : plane_in, row = yrole ? W : in_w;          // floats per plane / per row of the tensor this wave walks
        const unsigned long long base = yrole ? reinterpret_cast<unsigned long long>(dy)
                                              : reinterpret_cast<unsigned long long>(x) - (unsigned long long)(in_w + 1) * 4ull;
        const long long bytes = (long long)N * planes * pl_sz * 4 + (yrole ? 0 : (long long)(in_w + 1) * 4);
        sin[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)base);
        sin[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)(base >> 32));
        sin[2] = __builtin_amdgcn_readfirstlane(TH);
        sin[3] = __builtin_amdgcn_readfirstlane(TH - ty0);
        // from the end of an image's walk (H rows below the start of its first plane) to the start of the next image
        sin[4] = __builtin_amdgcn_readfirstlane((int)(((long long)planes * pl_sz - (long long)H * row) * 4));
        sin[5] = __builtin_amdgcn_readfirstlane(CPR - q0);
        sin[6] = __builtin_amdgcn_readfirstlane((int)(((long long)n0 * planes * pl_sz + (long long)((yrole ? 0 : in_oy) + 4 * ty0) * row +
                                                       (yrole ? 0 : in_ox) + 16 * q0) * 4));
        sin[7] = __builtin_amdgcn_readfirstlane((wsb != nullptr && cb == 0) ? 1 : 0);
        sin[8] = __builtin_amdgcn_readfirstlane((int)bytes);
        sin[9] = __builtin_amdgcn_readfirstlane(CPR);
        sin[10] = __builtin_amdgcn_readfirstlane(nch);
        sin[11] = __builtin_amdgcn_readfirstlane((4 * (yrole ? W : in_w) - W) * 4);      // from the end of a tile row's walk to the next tile row
        // EXEC of the edge-column loads of a chunk that starts (waves 0-1: not the lanes of tile 0) / ends (waves 2-3: tile 3) a tile row
        sin[12] = __builtin_amdgcn_readfirstlane(halo ? -1 : wave < 2 ? (int)0xEEEEEEEEu : wave < 4 ? 0x77777777 : -1);
        sin[13] = sin[12];
        sin[14] = __builtin_amdgcn_readfirstlane(wave < 2 ? 0 : wave < 4 ? 1 : 2);
        sin[15] = __builtin_amdgcn_readfirstlane(halo ? (int)bytes : 0);      // size word of the loads of rows -1 / H: 0 = nothing is read
    }
    // the statement ends with G^T m G of the lane's four (k, c) pairs (accumulator registers R = 0..3 -> v[9 R : 9 R + 8]): nothing of the 144
    // accumulators crosses a statement boundary (the register allocator copied and spilled them between separate statements)
    f32x32 o0;
    f4v o1;
    float bsum;
    asm volatile(TAI_W43_LOOP_ASM_WRW
                 : "={v[0:31]}"(o0), "={v[32:35]}"(o1), "={v98}"(bsum)
                 : "{v[46:61]}"(vin), "{s[48:63]}"(sin)
                 : TAI_W43_WRW_CLOBBERS);
    const int kq = lane >> 4, l16 = lane & 15;
    const int c = cb * TN + wn * 16 + l16;
    const long long ts = (long long)Kpad * Cpad;
    float* out = ws + (long long)sp * 9 * ts + (long long)(kb * TM + ch0 + 4 * kq) * Cpad + c;
#pragma unroll
    for (int i = 0; i < 36; ++i) out[(long long)(i % 9) * ts + (long long)(i / 9) * Cpad] = i < 32 ? o0[i] : o1[i - 32];
    // ---- bias gradient partials per (split, output channel)
    if (wsb != nullptr && cb == 0 && yrole) {          // the four tile lanes of an output channel are neighbours
        float v = bsum;
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        if ((lane & 3) == 0) wsb[(long long)sp * Kpad + kb * TM + 16 * (wave & 3) + (lane >> 2)] = v;
    }
}

}  // namespace wino43
