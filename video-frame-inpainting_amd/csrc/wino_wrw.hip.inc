// Weight gradient of the 3x3 stride-1 "same" convolution, fp32, in the Winograd F(2x2, 3x3) domain on the fp32 MFMA pipe
// (included by sepconv_capi.hip after wino_conv.hip.inc, whose MFMA helpers and conventions it shares).
//
// The training step (src/train.py:147-169 -> environments.py:348-355) back-propagates through ~350 convolutions; their
// weight gradients were MIOpen's implicit-GEMM kernels in NHWC (120 ms of a 437 ms step, plus 25 ms of layout transposes
// around them).  With  Y = A^T [ U .* V ] A,  U = G g G^T,  V = B^T d B  per 2x2-output tile,
//     dL/dU[pos] = sum over tiles of  (A dY A^T)[pos] * V[pos]        -- 16 independent GEMMs  [K x tiles] x [tiles x C]
//     dL/dg      = G^T (dL/dU) G
// i.e. the same 2.25x saving in multiplies as the forward kernel, with the TILES as the reduction dimension.
//
// Work decomposition: a workgroup (4 waves, one per SIMD, 512 registers each) owns a 64 x 64 block of (output channel k,
// input channel c) for ALL 16 transform positions -- wave (wm, wn) the 32 x 32 block, 16 accumulators x 16 registers in
// AGPRs -- and a contiguous run of tiles (a "split"; 256 workgroups in total at the bi-TAI shapes).  The run is consumed
// in chunks of 8 tiles (4 MFMA k-steps of 2): per chunk every thread loads and transforms two 4x4 input patches (B^T d B,
// as in the forward kernel) and two 2x2 output-gradient tiles (A dY A^T: 6 packed adds, two signs deferred to the epilogue)
// and writes them to LDS in MFMA operand order, double-buffered, one barrier per chunk.  Lanes are (channel lane/8, tile
// lane%8): the 8 tiles of a chunk lie in one tile row, so a patch row is 64 contiguous bytes per channel and the outer
// columns come from the neighbouring lanes (DPP) except at the two ends of the run.
// The output-gradient pixels also pass through the kernel exactly once per (k, split): their sums are the bias gradient.
// Epilogue: G^T m G per lane (all 16 positions of one (k, c) live in one lane), 9 taps to ws[split][tap][Kpad][Cpad];
// wrw_reduce sums the splits in a fixed order (no atomics: the gradient is reproducible) into dW [K, C, 3, 3].
//
// LDS operand order, both operands: [position pair q][kk][h][row 0..63][sl][e] with the reduction slot of tile t of the
// chunk = 2 * (2h + sl) + kk, rows of 4 floats, blocks of 64 rows padded to 288 floats so that the 8-byte writes of a wave
// (8 rows x 8 tiles) spread over all 64 banks.

namespace wino {
namespace wrw {

constexpr int BS = 288;                      // floats per [q][kk][h] block: 64 rows x 4 + 32
constexpr int REGION = 32 * BS;              // one operand, one stage
constexpr int STAGE = 2 * REGION;            // A (transformed dY) then B (transformed x): 18432 floats
constexpr int LDS_BYTES = 2 * STAGE * 4;     // 147,456 B
constexpr int CT = 8;                        // tiles per chunk

// PAIR (W % 32 == 0): chunks come in pairs over 16 consecutive tiles -- the even tiles are one chunk, the odd tiles the
// next -- and a lane loads 16 bytes of a row: its tile of either chunk.  Every load instruction then takes whole 128-byte
// lines (8 channels x 128 B) instead of half lines whose other half is wanted a chunk later: with 64 B pieces the L2 missed
// 3.4x the algorithmic bytes on the 64-channel 128 x 128 layers (plane strides of 64 KB land the channels in the same sets;
// profiles/r02_wrw_counters.txt) and the kernel ran at the memory system's pace.  One register buffer holds a pair: its
// odd-tile half is transformed one chunk after its even-tile half, then the next pair's loads start.
// DBG & WRW_RAGGED: any H and W (wrw_plan sends there every shape but even H with W % 16 == 0).  The kernel computes what the
// host-side widening computes: both planes zero-extended to an even number of rows and roundup(W, 16) columns, so every chunk of
// 8 tiles still lies in one tile row.  Nothing is copied: rows past H and columns past W (past the input plane, for x) are
// out-of-range offsets of the patch and output-gradient loads, i.e. zeros; row starts are then only 4-byte aligned, so the
// 8-byte loads become two 4-byte loads.  The extension is exact: the added output-gradient pixels are zeros and contribute
// nothing, the added input pixels are the convolution's own zero padding.  (A flag of DBG, not a third template parameter: the
// even-shape instantiations keep their names and their instruction streams; the remaining bits of DBG are the stamp level.)
constexpr int WRW_RAGGED = 4;
template <int DBG, bool PAIR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void conv3x3_wrw(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ ws, float* __restrict__ wsb, int N,
                 int C, int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, int kblocks, int cblocks,
                 int chunks_per_split, int nchunks_total, long long* __restrict__ stamps) {
    constexpr bool RAGGED = (DBG & WRW_RAGGED) != 0;
    constexpr int STAMPS = DBG & 3;
    static_assert(!(RAGGED && PAIR), "the ragged form reads single chunks");
    long long t_entry = 0, t_pro = 0, t_loop = 0;
    if (STAMPS) t_entry = __builtin_readcyclecounter();
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int bid = blockIdx.x;
    const int kb = bid % kblocks, cb = (bid / kblocks) % cblocks, sp = bid / (kblocks * cblocks);
    // (RAGGED: the tile grid of the zero-extended planes, H + 1 rows for an odd H, W rounded up to 16 columns)
    const int TH = RAGGED ? (H + 1) >> 1 : H >> 1, TW = RAGGED ? ((W + 15) & ~15) >> 1 : W >> 1;
    const long long plane = (long long)H * W;
    // The input plane is in_h x in_w with the pixel under output (0, 0) at (in_oy, in_ox): (H, W, 0, 0) for an ordinary tensor,
    // whose border is the zero padding; a tensor that carries its own halo (the shifted-copy stack of the 5x5 / 7x7 layers,
    // tai_conv_shift_stack: (H + 2, W + 4, 1, 2)) is read inside it and nothing is padded.
    const long long plane_in = (long long)in_h * in_w;
    const int c_first = sp * chunks_per_split;
    const int nch = min(chunks_per_split, nchunks_total - c_first);
    const int last = nch - 1;

    // ---- load role: lane = (channel cl, tile t of the chunk); two channels per lane (p = 0, 1: + 8)
    constexpr unsigned OUT_OF_RANGE = 0x80000000u;          // both tensors are < 2^31 bytes (checked by the launcher)
    const int t = lane & 7, cl = lane >> 3;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)((long long)N * C * plane_in * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t yrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), 0, (int)((long long)N * K * plane * 4), 0x00020000);
    unsigned vmid[2], vleft[2], vright[2], vdy[2];          // byte offsets of the lane's channel and tile column; the image,
#pragma unroll                                               // row and first column of the chunk ride in the scalar offset
    for (int p = 0; p < 2; ++p) {
        const int cx = cb * 64 + 16 * wave + 8 * p + cl, ky = kb * 64 + 16 * wave + 8 * p + cl;
        vmid[p] = cx < C ? (unsigned)(((long long)cx * plane_in + (PAIR ? 4 : 2) * t) * 4) : OUT_OF_RANGE;
        vleft[p] = (cx < C && t == 0) ? vmid[p] : OUT_OF_RANGE;      // (read with the scalar offset 4 bytes lower: a voffset of -4 is out of range)
        vright[p] = (cx < C && t == 7) ? vmid[p] + (PAIR ? 16u : 8u) : OUT_OF_RANGE;
        vdy[p] = ky < K ? (unsigned)(((long long)ky * plane + (PAIR ? 4 : 2) * t) * 4) : OUT_OF_RANGE;
    }
    const float mask_left = t > 0 ? 1.f : 0.f, mask_right = t < 7 ? 1.f : 0.f;
    // position of the next chunk to load (wave-uniform): image, tile row, first tile column
    int ln, lty, ltx;
    {
        const int tile0 = c_first * CT;
        const int n0 = tile0 / (TH * TW), rem = tile0 - n0 * TH * TW, ty0 = rem / TW;
        ln = __builtin_amdgcn_readfirstlane(n0);
        lty = __builtin_amdgcn_readfirstlane(ty0);
        ltx = __builtin_amdgcn_readfirstlane(rem - ty0 * TW);
    }
    constexpr int LT = PAIR ? 2 * CT : CT;                  // tiles per load step
    int loaded = 0;                                          // index (within the split) of the chunk (pair) at (ln, lty, ltx)
    auto advance = [&]() {
        // past the end of the split: the position stays on the last chunk and the output gradient reads as zeros -- the
        // loop below runs chunks in pairs, and the phantom chunk of an odd split adds nothing
        // (selects, not branches: the chunk loop has to stay one basic block, or the register allocator splits the
        // accumulators' live ranges around the inner blocks and copies all 256 of them through scratch every iteration)
        const int go = loaded < (PAIR ? (nch >> 1) - 1 : last) ? 1 : 0;
        const int nx = ltx + LT, w1 = nx >= TW ? 1 : 0;
        const int ny = lty + w1, w2 = ny >= TH ? 1 : 0;
        ltx = go ? (w1 ? 0 : nx) : ltx;
        lty = go ? (w2 ? 0 : ny) : lty;
        ln += go & w2;
        ++loaded;
    };

    float2 dm[2][2][4], dlr[2][2][4], gy[2][2][2];           // [register buffer][patch][row]
    // PAIR: one buffer for the pair of chunks: a row's four pixels (tile 2t: x, y; tile 2t+1: z, w), the run's outer columns
    float4 pm[2][4], pg[2][2];
    float2 pe[2][4];
    typedef float pvf4 __attribute__((ext_vector_type(4)));
    auto pair_load_x_row = [&](int p, int i) {
        const int yy = 2 * lty - 1 + i + in_oy;
        const bool rowok = yy >= 0 && yy < in_h;             // outside the input plane: the zero padding
        const int yyc = min(max(yy, 0), in_h - 1);
        const int col = 2 * ltx + in_ox;                     // the run's first pixel column in the plane
        const int soff = (int)((((long long)ln * C) * plane_in + (long long)yyc * in_w + col) * 4);
        const unsigned vm = rowok ? vmid[p] : OUT_OF_RANGE;
        const unsigned vl = (rowok && col > 0) ? vleft[p] : OUT_OF_RANGE;
        const unsigned vr = (rowok && col + 2 * LT < in_w) ? vright[p] : OUT_OF_RANGE;
        // (auto: the builtin returns a GCC-style vector of 4 unsigned; converting that to an ext_vector_type broadcasts element 0)
        const auto q = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, vm, soff, 0);
        static_assert(sizeof(q) == 16, "16-byte buffer load");
        const pvf4 qf = __builtin_bit_cast(pvf4, q);
        pm[p][i] = make_float4(qf.x, qf.y, qf.z, qf.w);
        pe[p][i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, vl, col > 0 ? soff - 4 : soff, 0));
        pe[p][i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, vr, soff, 0));
    };
    auto pair_load_dy_row = [&](int p, int r) {
        const int soff = (int)((((long long)ln * K) * plane + (long long)(2 * lty + r) * W + 2 * ltx) * 4);
        // (past the split's last pair: zeros -- the last chunk transforms a pair nobody multiplies, and the bias sum must not see it)
        const auto q = __builtin_amdgcn_raw_buffer_load_b128(yrsrc, loaded < (nch >> 1) ? vdy[p] : OUT_OF_RANGE, soff, 0);
        const pvf4 qf = __builtin_bit_cast(pvf4, q);
        pg[p][r] = make_float4(qf.x, qf.y, qf.z, qf.w);
    };
    auto load_x_row = [&](auto buf_c, int p, int i) {
        constexpr int buf = decltype(buf_c)::value;
        const int yy = 2 * lty - 1 + i + in_oy;
        const bool rowok = yy >= 0 && yy < in_h;             // outside the input plane: the zero padding
        const int yyc = min(max(yy, 0), in_h - 1);
        const int col = 2 * ltx + in_ox;                     // the run's first pixel column in the plane
        const int soff = (int)((((long long)ln * C) * plane_in + (long long)yyc * in_w + col) * 4);
        const unsigned vm = rowok ? vmid[p] : OUT_OF_RANGE;
        const unsigned vl = (rowok && col > 0) ? vleft[p] : OUT_OF_RANGE;
        const unsigned vr = (rowok && col + 2 * CT < in_w) ? vright[p] : OUT_OF_RANGE;
        if constexpr (RAGGED) {        // columns past the input plane read as zeros
            const unsigned vm0 = col + 2 * t < in_w ? vm : OUT_OF_RANGE, vm1 = col + 2 * t + 1 < in_w ? vm + 4u : OUT_OF_RANGE;
            dm[buf][p][i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, vm0, soff, 0));
            dm[buf][p][i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, vm1, soff, 0));
        } else {
            dm[buf][p][i] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(xrsrc, vm, soff, 0));
        }
        dlr[buf][p][i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, vl, col > 0 ? soff - 4 : soff, 0));
        dlr[buf][p][i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, vr, soff, 0));
    };
    auto load_dy_row = [&](auto buf_c, int p, int r) {
        constexpr int buf = decltype(buf_c)::value;
        const int soff = (int)((((long long)ln * K) * plane + (long long)(2 * lty + r) * W + 2 * ltx) * 4);
        if constexpr (RAGGED) {        // rows past H and columns past W read as zeros
            const bool ok = loaded <= last && 2 * lty + r < H;
            const int c0 = 2 * ltx + 2 * t;
            const unsigned v0 = (ok && c0 < W) ? vdy[p] : OUT_OF_RANGE, v1 = (ok && c0 + 1 < W) ? vdy[p] + 4u : OUT_OF_RANGE;
            gy[buf][p][r].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yrsrc, v0, soff, 0));
            gy[buf][p][r].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yrsrc, v1, soff, 0));
        } else {
            gy[buf][p][r] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(yrsrc, loaded <= last ? vdy[p] : OUT_OF_RANGE, soff, 0));
        }
    };
    auto load_all = [&](auto buf_c) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int i = 0; i < 4; ++i) load_x_row(buf_c, p, i);
#pragma unroll
            for (int r = 0; r < 2; ++r) load_dy_row(buf_c, p, r);
        }
    };

    // ---- transforms.  x: B^T d B exactly as in conv3x3 (rows on register pairs, outer columns through DPP).
    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f tmid[2][4], tout[2][4];
    float4 wx[8], wy[8];                        // per position pair: (patch 0 pair, patch 1 pair)
    auto transform_x_rows = [&](auto buf_c, int p) {
        constexpr int buf = decltype(buf_c)::value;
        v2f mid[4], out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 m = dm[buf][p][i];
            float left = dlr[buf][p][i].x, right = dlr[buf][p][i].y;
            asm("v_fmac_f32_dpp %0, %1, %2 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(left) : "v"(m.y), "v"(mask_left));
            asm("v_fmac_f32_dpp %0, %1, %2 wave_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(right) : "v"(m.x), "v"(mask_right));
            mid[i] = v2f{m.x, m.y};
            out[i] = v2f{left, right};
        }
        tmid[p][0] = mid[0] - mid[2]; tout[p][0] = out[0] - out[2];
        tmid[p][1] = mid[1] + mid[2]; tout[p][1] = out[1] + out[2];
        tmid[p][2] = mid[2] - mid[1]; tout[p][2] = out[2] - out[1];
        tmid[p][3] = mid[1] - mid[3]; tout[p][3] = out[1] - out[3];
    };
    auto transform_x_cols = [&](int p) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v2f vo, vm;
            asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(vo) : "v"(tout[p][r]), "v"(tmid[p][r]));
            asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(vm) : "v"(tmid[p][r]));
            if (p == 0) { wx[2 * r].x = vo.x; wx[2 * r].y = vo.y; wx[2 * r + 1].x = vm.x; wx[2 * r + 1].y = vm.y; }
            else        { wx[2 * r].z = vo.x; wx[2 * r].w = vo.y; wx[2 * r + 1].z = vm.x; wx[2 * r + 1].w = vm.y; }
        }
    };
    // PAIR: part 0 = the even tile of the lane (pixels x, y; left neighbour = the previous lane's w, right = own z),
    // part 1 = the odd tile (z, w; left = own y, right = the next lane's x); the run's two ends from the outer loads.
    auto pair_transform_x_rows = [&](auto part_c, int p) {
        constexpr int part = decltype(part_c)::value;
        v2f mid[4], out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 m = pm[p][i];
            if (part == 0) {
                float left = pe[p][i].x;
                asm("v_fmac_f32_dpp %0, %1, %2 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(left) : "v"(m.w), "v"(mask_left));
                mid[i] = v2f{m.x, m.y};
                out[i] = v2f{left, m.z};
            } else {
                float right = pe[p][i].y;
                asm("v_fmac_f32_dpp %0, %1, %2 wave_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(right) : "v"(m.x), "v"(mask_right));
                mid[i] = v2f{m.z, m.w};
                out[i] = v2f{m.y, right};
            }
        }
        tmid[p][0] = mid[0] - mid[2]; tout[p][0] = out[0] - out[2];
        tmid[p][1] = mid[1] + mid[2]; tout[p][1] = out[1] + out[2];
        tmid[p][2] = mid[2] - mid[1]; tout[p][2] = out[2] - out[1];
        tmid[p][3] = mid[1] - mid[3]; tout[p][3] = out[1] - out[3];
    };
    float bsum[2] = {0.f, 0.f};
    // dY: A dY A^T with A = [[1,0],[1,1],[1,-1],[0,-1]].  Rows T0 = (a,b), T1 = (a+c,b+d), T2 = (a-c,b-d), T3 = -(c,d); a row
    // (p,q) becomes (p, p+q, p-q, -q).  The two negations (row 3, column 3) are left out here and applied as signs of the
    // accumulated positions in the epilogue, so the outer pair (columns 0, 3) is the row itself.
    auto transform_dy_rows = [&](int p, const float2 r0, const float2 r1) {
        bsum[p] += (r0.x + r0.y) + (r1.x + r1.y);             // bias gradient: every output-gradient pixel passes here once
        const v2f T[4] = {v2f{r0.x, r0.y}, v2f{r0.x + r1.x, r0.y + r1.y}, v2f{r0.x - r1.x, r0.y - r1.y}, v2f{r1.x, r1.y}};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const v2f vo = T[r], vm = v2f{T[r].x + T[r].y, T[r].x - T[r].y};
            if (p == 0) { wy[2 * r].x = vo.x; wy[2 * r].y = vo.y; wy[2 * r + 1].x = vm.x; wy[2 * r + 1].y = vm.y; }
            else        { wy[2 * r].z = vo.x; wy[2 * r].w = vo.y; wy[2 * r + 1].z = vm.x; wy[2 * r + 1].w = vm.y; }
        }
    };
    auto transform_dy = [&](auto buf_c, int p) {
        constexpr int buf = decltype(buf_c)::value;
        transform_dy_rows(p, gy[buf][p][0], gy[buf][p][1]);
    };
    auto pair_transform_dy = [&](auto part_c, int p) {
        constexpr int part = decltype(part_c)::value;
        const float4 g0 = pg[p][0], g1 = pg[p][1];
        if (part == 0) transform_dy_rows(p, make_float2(g0.x, g0.y), make_float2(g1.x, g1.y));
        else transform_dy_rows(p, make_float2(g0.z, g0.w), make_float2(g1.z, g1.w));
    };
    // LDS writes: the lane's tile t is reduction slot (kk, h, sl) = (t & 1, t >> 2, (t >> 1) & 1); row = 16 * wave + 8 p + cl
    // (byte addresses, one base register per stage and operand, opaque to the optimiser like the read addresses below)
    typedef __attribute__((address_space(3))) v2f lds_v2f;
    unsigned wbase[2][2];                       // [stage][region: 0 transformed dY, 1 transformed x]
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int rg = 0; rg < 2; ++rg) {
            wbase[st][rg] = (unsigned)((st * STAGE + rg * REGION + ((t & 1) * 2 + (t >> 2)) * BS + (16 * wave + cl) * 4 + ((t >> 1) & 1) * 2) * 4);
            asm volatile("" : "+v"(wbase[st][rg]));
        }
    auto write_pair = [&](int stage, int region, int q, const float4& v) {
        const unsigned dst = wbase[stage][region] + (unsigned)(q * 4 * BS * 4);
        // two ds_write_b64 (patch 1: 8 rows = 128 bytes further), not the ds_write2_b64 the compiler merges them into: the
        // pair's second element lands 32 banks from the first, on top of the h = 1 lanes' first elements
        const v2f lo = v2f{v.x, v.y}, hi = v2f{v.z, v.w};
        asm volatile("ds_write_b64 %0, %1\n\tds_write_b64 %0, %2 offset:128" : : "v"(dst), "v"(lo), "v"(hi) : "memory");
    };

    const std::integral_constant<int, 0> B0;
    const std::integral_constant<int, 1> B1;
    // ---- prologue: chunk 0 loaded, transformed and written to stage 0; then the loads of chunks 1 and 2 start and the
    // accumulators are cleared while they travel.  (All three chunks in flight at once, as conv3x3 does it, needs a third
    // register buffer: with the accumulators live as well the allocator parks them in scratch.)
    if constexpr (PAIR) {        // pair 0 loaded; its even-tile half goes to stage 0 (the odd-tile half during chunk 0)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int i = 0; i < 4; ++i) pair_load_x_row(p, i);
#pragma unroll
            for (int r = 0; r < 2; ++r) pair_load_dy_row(p, r);
        }
        advance();
        pair_transform_x_rows(B0, 0); transform_x_cols(0);
        pair_transform_x_rows(B0, 1); transform_x_cols(1);
        pair_transform_dy(B0, 0); pair_transform_dy(B0, 1);
#pragma unroll
        for (int q = 0; q < 8; ++q) { write_pair(0, 0, q, wy[q]); write_pair(0, 1, q, wx[q]); }
        __builtin_amdgcn_sched_barrier(0);
    } else {
        load_all(B1); advance();
        transform_x_rows(B1, 0); transform_x_cols(0);
        transform_x_rows(B1, 1); transform_x_cols(1);
        transform_dy(B1, 0); transform_dy(B1, 1);
#pragma unroll
        for (int q = 0; q < 8; ++q) { write_pair(0, 0, q, wy[q]); write_pair(0, 1, q, wx[q]); }
        __builtin_amdgcn_sched_barrier(0);
        load_all(B1); advance();
        load_all(B0); advance();
        __builtin_amdgcn_sched_barrier(0);
    }
    f16v acc[16];
#pragma unroll
    for (int f = 0; f < 16; ++f)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[f][j] = 0.f;
#pragma unroll
    for (int f = 0; f < 16; ++f) asm volatile("" : "+a"(acc[f]));
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (STAMPS) t_pro = __builtin_readcyclecounter();

    // LDS byte addresses (dynamic LDS starts at address 0) of the lane's operand rows: [kk = lane / 32][h = 0][row], one base
    // register per operand and stage, every group's block an immediate offset (< 64 KB).  Kept opaque to the optimiser:
    // given the arithmetic it folds stage and region into 32 separate address registers and spills them.
    typedef float vf4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const vf4 lds_f4;
    auto lds_read4 = [](unsigned addr) { const vf4 v = *reinterpret_cast<lds_f4*>(addr); return make_float4(v.x, v.y, v.z, v.w); };
    unsigned abase[2], bbase[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        abase[st] = (unsigned)((st * STAGE + (lane >> 5) * 2 * BS + (wm * 32 + (lane & 31)) * 4) * 4);
        bbase[st] = (unsigned)((st * STAGE + REGION + (lane >> 5) * 2 * BS + (wn * 32 + (lane & 31)) * 4) * 4);
        asm volatile("" : "+v"(abase[st]), "+v"(bbase[st]));
    }

    // One chunk: 64 MFMAs in 16 groups of 4, as in conv3x3.  Transform the operands of chunk ch+1 (register buffer `nb`)
    // after groups 0-3, write them to the other LDS stage in groups 4-11, start the loads of chunk ch+3 into `nb` in
    // groups 8-15.
    auto chunk = [&](int ch, auto stage_c, auto nb_c) {
        constexpr int stage = decltype(stage_c)::value;
        constexpr int nb = decltype(nb_c)::value;
        float4 a[2], b[2];
        a[0] = lds_read4(abase[stage]);
        b[0] = lds_read4(bbase[stage]);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int g = j >> 1;
            const int f0 = 4 * (g >> 1) + (g & 1), f1 = 4 * (g >> 1) + 3 - (g & 1);
            mfma1(acc[f0], a[j & 1], b[j & 1]);
            __builtin_amdgcn_sched_barrier(0);
            if (j < 15) {
                const unsigned blk = (unsigned)((((j + 1) >> 1) * 4 + ((j + 1) & 1)) * BS * 4);
                a[(j + 1) & 1] = lds_read4(abase[stage] + blk);
                b[(j + 1) & 1] = lds_read4(bbase[stage] + blk);
            }
            if (j >= 4 && j < 8) { write_pair(stage ^ 1, 1, 2 * (j - 4), wx[2 * (j - 4)]); write_pair(stage ^ 1, 1, 2 * (j - 4) + 1, wx[2 * (j - 4) + 1]); }
            if (j >= 8 && j < 12) { write_pair(stage ^ 1, 0, 2 * (j - 8), wy[2 * (j - 8)]); write_pair(stage ^ 1, 0, 2 * (j - 8) + 1, wy[2 * (j - 8) + 1]); }
            if constexpr (PAIR) {
                // nb_c 1: this is the pair's first chunk -- its odd-tile half is transformed in groups 0-3 below, then the
                // buffer is free and the next pair's loads start, in the order the next chunk consumes them
                if (nb == 1 && j >= 4 && j < 8) { pair_load_x_row((j - 4) >> 1, 2 * ((j - 4) & 1)); pair_load_x_row((j - 4) >> 1, 2 * ((j - 4) & 1) + 1); }
                if (nb == 1 && j >= 8 && j < 10) { pair_load_dy_row(j - 8, 0); pair_load_dy_row(j - 8, 1); }
            } else {
                if (j >= 4 && j < 12) load_x_row(nb_c, (j - 4) >> 2, (j - 4) & 3);
                if (j >= 4 && j < 8) load_dy_row(nb_c, (j - 4) >> 1, (j - 4) & 1);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma3(acc[f0], acc[f1], a[j & 1], b[j & 1]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (PAIR) {       // first chunk of a pair: the pair's odd tiles feed the next chunk; second: the next pair's even tiles
                if (j == 0) pair_transform_x_rows(nb_c, 0);
                if (j == 1) transform_x_cols(0);
                if (j == 2) pair_transform_x_rows(nb_c, 1);
                if (j == 3) { transform_x_cols(1); pair_transform_dy(nb_c, 0); pair_transform_dy(nb_c, 1); }
            } else {
                if (j == 0) transform_x_rows(nb_c, 0);
                if (j == 1) transform_x_cols(0);
                if (j == 2) transform_x_rows(nb_c, 1);
                if (j == 3) { transform_x_cols(1); transform_dy(nb_c, 0); transform_dy(nb_c, 1); }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (STAMPS == 2 && ch >= 2 && ch < 4 && tid == 0) stamps[64 * (long long)blockIdx.x + 30 + 16 * (ch - 2) + j] = __builtin_readcyclecounter();
        }
        if (!PAIR || nb == 1) advance();
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (STAMPS && tid == 0 && ch < 26) stamps[64 * (long long)blockIdx.x + 4 + ch] = __builtin_readcyclecounter();
    };
    for (int ch = 0; ch < nch; ch += 2) {       // (a separate tail chunk makes the allocator route accumulators through scratch)
        chunk(ch, B0, B1);
        chunk(ch + 1, B1, B0);
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    if (STAMPS) t_loop = __builtin_readcyclecounter();

    // ---- epilogue: G^T m G per lane.  acc[4r + col][j]: transform position (r, col) of (k, c) with
    // k = 8 (j / 4) + 4 (lane / 32) + j % 4, c = lane % 32 of the wave's block; positions of row 3 or column 3 (not both)
    // carry the deferred minus sign.  G^T = [[1, .5, .5, 0], [0, .5, -.5, 0], [0, .5, .5, 1]].
    const int Kpad = kblocks * 64, Cpad = cblocks * 64;
    const int half = lane >> 5;
    float* out = ws + (long long)sp * 9 * Kpad * Cpad + (long long)(kb * 64 + wm * 32 + 4 * half) * Cpad + cb * 64 + wn * 32 + (lane & 31);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        f16v n[4];
#pragma unroll
        for (int col = 0; col < 4; ++col) {
            // rows of G^T applied to column `col`: m0, m1, m2 as accumulated, m3 negated (the deferred row sign)
            if (a == 0) n[col] = acc[col] + 0.5f * (acc[4 + col] + acc[8 + col]);
            if (a == 1) n[col] = 0.5f * (acc[4 + col] - acc[8 + col]);
            if (a == 2) n[col] = 0.5f * (acc[4 + col] + acc[8 + col]) - acc[12 + col];
            __builtin_amdgcn_sched_barrier(0);
        }
        // columns: n3 negated (the deferred column sign)
        const f16v w0 = n[0] + 0.5f * (n[1] + n[2]), w1 = 0.5f * (n[1] - n[2]), w2 = 0.5f * (n[1] + n[2]) - n[3];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float* o = out + (long long)(8 * (j >> 2) + (j & 3)) * Cpad;
            o[(long long)(3 * a + 0) * Kpad * Cpad] = w0[j];
            o[(long long)(3 * a + 1) * Kpad * Cpad] = w1[j];
            o[(long long)(3 * a + 2) * Kpad * Cpad] = w2[j];
        }
    }
    // bias gradient partials: sum the 8 tile lanes of each channel, one value per (split, k) from the c-block 0 workgroups
    if (wsb != nullptr && cb == 0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float v = bsum[p];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            if (t == 0) wsb[(long long)sp * Kpad + kb * 64 + 16 * wave + 8 * p + cl] = v;
        }
    }
    if (STAMPS && tid == 0) {
        long long* st = stamps + 64 * (long long)blockIdx.x;
        st[0] = t_entry; st[1] = t_pro; st[2] = t_loop; st[3] = __builtin_readcyclecounter();
    }
}

// dW[k][c][tap] = sum over splits of ws[split][tap][k][c].  A workgroup handles 64 consecutive c of one (tap, k) row:
// thread (g, i) sums the splits g, g + 4, ... of column i (four independent loads in flight per thread), the four partial
// sums are combined through LDS in a fixed order.
__global__ __launch_bounds__(256)
void wrw_reduce(const float* __restrict__ ws, float* __restrict__ dw, const float* __restrict__ wsb, float* __restrict__ dbias,
                int K, int C, int Kpad, int Cpad, int splits) {
    __shared__ float part[4][64];
    const int i = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int cblk = (C + 63) / 64;
    const long long rows = 9LL * K * cblk;
    const long long split_stride = 9LL * Kpad * Cpad;
    // dbias[k] = sum over splits of wsb[split][k]: the last Kpad / 64 workgroups, 64 channels each, same scheme
    if (dbias != nullptr && (int)(gridDim.x - 1 - blockIdx.x) < Kpad / 64) {
        const int k = (int)(gridDim.x - 1 - blockIdx.x) * 64 + i;
        float sb = 0.f;
        for (int sp = g; sp < splits; sp += 4) sb += wsb[(long long)sp * Kpad + k];
        part[g][i] = sb;
        __syncthreads();
        if (g == 0 && k < K) dbias[k] = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
        __syncthreads();
    }
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const int cb = (int)(row % cblk);
        const int k = (int)((row / cblk) % K);
        const int tap = (int)(row / ((long long)cblk * K));
        const int c = cb * 64 + i;
        const float* src = ws + ((long long)tap * Kpad + k) * Cpad + c;          // c < Cpad always
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int sp = g;
        for (; sp + 12 < splits; sp += 16) {
            s0 += src[(long long)sp * split_stride];
            s1 += src[(long long)(sp + 4) * split_stride];
            s2 += src[(long long)(sp + 8) * split_stride];
            s3 += src[(long long)(sp + 12) * split_stride];
        }
        for (; sp < splits; sp += 4) s0 += src[(long long)sp * split_stride];
        __syncthreads();                                   // part[] of the previous row has been read
        part[g][i] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (g == 0 && c < C) dw[((long long)k * C + c) * 9 + tap] = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
    }
}

}  // namespace wrw
}  // namespace wino
