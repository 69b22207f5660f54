// 3x3 stride-1 "same" convolution, fp32, as Winograd F(2x2, 3x3) on the fp32 MFMA pipe (included by sepconv_capi.hip).
//
// The MC-Net generator and the kernel network (src/models/mcnet/mcnet.py:63-294, src/models/tai/tai.py:244-348) are stacks
// of 3x3 stride-1 convolutions; at configs[1] they were 95 of the 132 ms of a bi-TAI forward on MIOpen, which runs them at 75-120
// TFLOP/s of direct-convolution flops.  F(2x2,3x3) turns a 3x3 convolution into 16 independent GEMMs (one per position
// of the 4x4 transform domain) with 2.25x fewer multiplies:
//     Y = A^T [ (G g G^T) .* (B^T d B) ] A          d: 4x4 input patch, g: 3x3 filter, Y: 2x2 outputs
// and the GEMMs run on v_mfma_f32_32x32x2_f32 (155 TFLOP/s measured on this chip, tools/mfma_microbench.hip).
//
// Work decomposition (one workgroup = 4 waves = one CU, 1 wave per SIMD so each wave owns 512 registers):
//   * a workgroup owns 64 output channels x 64 tiles (2x2 output pixels each; tiles are numbered (image, ty, tx) with tx
//     fastest, so a wave's 32 tiles are a contiguous run of a tile row and its stores coalesce);
//   * wave (wm, wn) owns the 32 x 32 block (channels wm, tiles wn) for ALL 16 transform positions: 16 accumulator
//     blocks x 16 registers = 256 accumulator registers.  Holding all 16 positions of one (channel, tile) in one lane
//     makes the inverse transform A^T m A pure per-lane register arithmetic -- no exchange;
//   * the reduction over input channels runs in chunks of 8: every thread loads two 4x4 patches, transforms them
//     (B^T d B: 8 DPP multiply-adds + 16 packed adds each) and writes the 16 transformed values to LDS in MFMA operand
//     order; the pre-transformed weights (tai_conv3x3_wino_transform_weights, same operand order) are copied global ->
//     LDS by global_load_lds_dwordx4, 16 bytes per lane, no registers; LDS is double-buffered (2 x 64 KB), one barrier
//     per chunk;
//   * MFMA operand order in LDS: [position pair q][k-half kk][k-step half h][row 0..63][k-step sl][pair element e],
//     input channel = 8*chunk + 2*(2h + sl) + kk.  The 16 transform positions are paired the way the packed fp32 adds of
//     the patch transform produce them -- per row r of the 4x4 domain the outer pair (4r, 4r+3) = q 2r and the middle
//     pair (4r+1, 4r+2) = q 2r+1 -- so ONE ds_read_b128 gives a lane its A (or B) operand of two positions for two MFMA
//     k-steps, and ONE ds_write_b128 stores a thread's two patches for a position pair.
//
// Entry points (sepconv_capi.hip): tai_conv3x3_wino_forward, _maxpool (second output: 2x2 max pool), _parts (input given
// as up to four channel parts), _window (input plane with its own halo: the 5x5 / 7x7 layers over shifted copies).
// conv3x3<..., TALL = true> is the same kernel on 128-channel x 32-tile workgroups (wave w owns channels 32w .. 32w+31 of
// the block and all 32 tiles): per chunk the workgroup transforms and writes to LDS half as many patches (one per thread)
// for the same 256 MFMAs and reads twice the weights, which cost nothing (DMA in the MFMA shadow); LDS 2 x 80 KB; for
// layers whose K is a multiple of 128.
// Measured: 185-268 TFLOP/s of direct-convolution flops on the bi-TAI shapes, 2.1-2.4x MIOpen's fp32 kernels; 0.65 of the
// fp32 MFMA peak over the workload's layer mix (bench.py roofline_conv); DESIGN.md 4.4 has the cycle accounting.
//
// v_mfma_f32_32x32x2_f32 operand map (wave64): A[m][k]: lane = 32*k + m;  B[k][n]: lane = 32*k + n;
// D[m][n]: lane = 32*((m / 4) % 2) + n, register = 4*(m / 8) + m % 4.

#include <type_traits>

namespace wino {

typedef float f16v __attribute__((ext_vector_type(16)));

// Divisors of the index arithmetic as multiply-high constants (host: wino_div_magic in sepconv_capi.hip): tiles per image, tiles
// per tile row, output-channel blocks.
struct DivMagic { unsigned m_tpi, s_tpi, m_tw, s_tw, m_kb, s_kb; };

constexpr int KC = 8;                        // input channels per chunk
constexpr int TM = 64, TN = 64;              // output channels x tiles per workgroup
constexpr int STAGE_FLOATS = 16 * 2 * (TM + TN) * 4;   // 16384 floats = 64 KB
constexpr int LDS_BYTES = 2 * STAGE_FLOATS * 4;
constexpr int TTM = 128, TTN = 32;           // the "tall" workgroup: 128 output channels x 32 tiles
constexpr int TSTAGE_FLOATS = 16 * 2 * (TTM + TTN) * 4;  // 20480 floats = 80 KB
constexpr int TLDS_BYTES = 2 * TSTAGE_FLOATS * 4;        // 160 KB: all of a CU's LDS

// U[chunk][q][kk][h][Kpad][sl][e] = (G g G^T)[position e of pair q] for output channel k, input channel
// c = 8*chunk + 2*(2h + sl) + kk; zero padded.  (32 runs of Kpad x 4 floats per chunk.)
__global__ void transform_weights(const float* __restrict__ w, float* __restrict__ U, int K, int C, int Kpad, int Cpad) {
    const long long total = (long long)Kpad * Cpad;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % Kpad), c = (int)(i / Kpad);
        float g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = (k < K && c < C) ? w[((long long)k * C + c) * 9 + a * 3 + b] : 0.f;
        float t[4][3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            t[0][b] = g[0][b];
            t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
            t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
            t[3][b] = g[2][b];
        }
        const int ch = c / KC, s = (c % KC) / 2, kk = c % 2, h = s >> 1, sl = s & 1;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float u0 = t[a][0], u1 = 0.5f * (t[a][0] + t[a][1] + t[a][2]), u2 = 0.5f * (t[a][0] - t[a][1] + t[a][2]),
                        u3 = t[a][2];
            const float u[4] = {u0, u1, u2, u3};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int q = 2 * a + ((b == 1 || b == 2) ? 1 : 0), e = (b >= 2) ? 1 : 0;    // pairs (0,3) and (1,2)
                U[(((((long long)ch * 8 + q) * 2 + kk) * 2 + h) * Kpad + k) * 4 + sl * 2 + e] = u[b];
            }
        }
    }
}

// The 256 accumulator registers of a wave must live in the AGPR half of its register file for the whole channel loop
// (the other half holds operands, patches and addresses).  Left to itself the register allocator moves accumulators
// back and forth and spills; the "a" constraint pins them.  Chained MFMAs on one accumulator (same opcode, SrcC == vDst)
// need no wait states between them; the reads in the epilogue are separated from the last MFMA by explicit s_nops.
// The four MFMAs of one half of a position pair (two accumulators x two k-steps, alternating: a dependent MFMA issued
// back to back costs ~4 cycles more than an independent one), issued as 1 + 3: LDS and memory instructions placed
// between the two parts issue in the shadow of the first MFMA (they are not vector-ALU work, so unlike VALU filler they
// do hide under a running MFMA).  The second form of the 3 also issues one 1 KB weight DMA (global_load_lds_dwordx4:
// LDS address = M0 + 16 * lane) the same way.  Operands a, b: (x, z) = the two k-steps of the first position, (y, w) of
// the second.
// Z (chunk 0 of a workgroup, PARTS != 2): the FIRST MFMA on an accumulator block takes the constant 0 as its C operand and only
// writes the block -- the 240 v_accvgpr_write of a zero-initialisation (1,020 cycles of the prologue, vector-ALU time that nothing
// overlaps: tools/wino_timeline.py) are never issued.  In a group, mfma1 is the first MFMA on c0 and the first instruction of mfma3
// the first on c1; the second half-group (odd j) accumulates as ever.  Block 5 (the bias) is the exception: it is initialised.
template <bool Z = false>
__device__ __forceinline__ void mfma1(f16v& c0, const float4& a, const float4& b) {
    if constexpr (Z) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, 0" : "=a"(c0) : "v"(a.x), "v"(b.x));
    else asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(c0) : "v"(a.x), "v"(b.x));
}
template <bool Z = false>
__device__ __forceinline__ void mfma3(f16v& c0, f16v& c1, const float4& a, const float4& b) {
    if constexpr (Z)
        asm volatile("v_mfma_f32_32x32x2_f32 %1, %2, %5, 0\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\t"
                     "v_mfma_f32_32x32x2_f32 %1, %4, %7, %1"
                     : "+a"(c0), "=&a"(c1) : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w));
    else
        asm volatile("v_mfma_f32_32x32x2_f32 %1, %2, %5, %1\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\t"
                     "v_mfma_f32_32x32x2_f32 %1, %4, %7, %1"
                     : "+a"(c0), "+a"(c1) : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w));
}
template <bool Z = false>
__device__ __forceinline__ void mfma3_dma(f16v& c0, f16v& c1, const float4& a, const float4& b, unsigned lane16, unsigned m0v,
                                          const char* gsrc) {
    if constexpr (Z)
        asm volatile("s_mov_b32 m0, %9\n\tv_mfma_f32_32x32x2_f32 %1, %2, %5, 0\n\t"
                     "global_load_lds_dwordx4 %8, %10\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\t"
                     "v_mfma_f32_32x32x2_f32 %1, %4, %7, %1"
                     : "+a"(c0), "=&a"(c1)
                     : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w), "v"(lane16), "s"(m0v), "s"(gsrc)
                     : "memory");
    else
        asm volatile("s_mov_b32 m0, %9\n\tv_mfma_f32_32x32x2_f32 %1, %2, %5, %1\n\t"
                     "global_load_lds_dwordx4 %8, %10\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\t"
                     "v_mfma_f32_32x32x2_f32 %1, %4, %7, %1"
                     : "+a"(c0), "+a"(c1)
                     : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w), "v"(lane16), "s"(m0v), "s"(gsrc)
                     : "memory");
}

template <bool Z = false>
__device__ __forceinline__ void mfma3_dma2(f16v& c0, f16v& c1, const float4& a, const float4& b, unsigned lane16, unsigned m0a,
                                           const char* ga, unsigned m0b, const char* gb) {
    if constexpr (Z)
        asm volatile("s_mov_b32 m0, %9\n\tv_mfma_f32_32x32x2_f32 %1, %2, %5, 0\n\t"
                     "global_load_lds_dwordx4 %8, %10\n\ts_mov_b32 m0, %11\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\t"
                     "global_load_lds_dwordx4 %8, %12\n\tv_mfma_f32_32x32x2_f32 %1, %4, %7, %1"
                     : "+a"(c0), "=&a"(c1)
                     : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w), "v"(lane16), "s"(m0a), "s"(ga), "s"(m0b), "s"(gb)
                     : "memory");
    else
        asm volatile("s_mov_b32 m0, %9\n\tv_mfma_f32_32x32x2_f32 %1, %2, %5, %1\n\t"
                     "global_load_lds_dwordx4 %8, %10\n\ts_mov_b32 m0, %11\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\t"
                     "global_load_lds_dwordx4 %8, %12\n\tv_mfma_f32_32x32x2_f32 %1, %4, %7, %1"
                     : "+a"(c0), "+a"(c1)
                     : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w), "v"(lane16), "s"(m0a), "s"(ga), "s"(m0b), "s"(gb)
                     : "memory");
}

// Displaced-read layers (PARTS == 2): the k x k filter is cut into blocks of 3 x 3 taps, zero past k, so in the LAST block
// row (column) the third tap row (column) is all zeros -- and with it, exactly, the fourth row (column) of the block's
// transformed 4 x 4 weights (G g G^T keeps g's third tap as its fourth component).  The MFMAs of those positions multiply
// by zeros: they are skipped, per chunk, by scalar branches INSIDE the asm blocks (a C++ branch around an asm block makes
// the accumulator a phi and the allocator copy AGPR sets).  zall: skip every MFMA of the group (transform row 3, groups
// 12-15); z1: skip the second position of an outer pair (transform column 3).  The weight DMA is always issued.
// Every variant is laid out so that the path WITHOUT skipping falls through: a forward branch that is not taken costs a
// cycle or two, a taken one (the `s_branch` over an else-part) cost the chunk 300-600 cycles at twelve groups per chunk
// (tools/kxk_timeline.py).  So the first position's MFMA goes first and the two MFMAs of the second position sit behind
// one forward branch; the accumulation order per accumulator is unchanged (results stay bit-identical).
__device__ __forceinline__ void mfma1z(f16v& c0, const float4& a, const float4& b, int zall) {
    asm volatile("s_cmp_lg_u32 %3, 0\n\ts_cbranch_scc1 1f\n\tv_mfma_f32_32x32x2_f32 %0, %1, %2, %0\n1:"
                 : "+a"(c0) : "v"(a.x), "v"(b.x), "s"(zall) : "scc");
}
__device__ __forceinline__ void mfma3z(f16v& c0, f16v& c1, const float4& a, const float4& b, int zall, int z1) {
    asm volatile("s_cmp_lg_u32 %8, 0\n\ts_cbranch_scc1 1f\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\t"
                 "s_cmp_lg_u32 %9, 0\n\ts_cbranch_scc1 1f\n\t"
                 "v_mfma_f32_32x32x2_f32 %1, %2, %5, %1\n\tv_mfma_f32_32x32x2_f32 %1, %4, %7, %1\n1:"
                 : "+a"(c0), "+a"(c1) : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w), "s"(zall), "s"(z1) : "scc");
}
__device__ __forceinline__ void mfma3z_dma(f16v& c0, f16v& c1, const float4& a, const float4& b, unsigned lane16, unsigned m0v,
                                           const char* gsrc, int z1) {
    asm volatile("s_mov_b32 m0, %9\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\tglobal_load_lds_dwordx4 %8, %10\n\t"
                 "s_cmp_lg_u32 %11, 0\n\ts_cbranch_scc1 1f\n\t"
                 "v_mfma_f32_32x32x2_f32 %1, %2, %5, %1\n\tv_mfma_f32_32x32x2_f32 %1, %4, %7, %1\n1:"
                 : "+a"(c0), "+a"(c1)
                 : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w), "v"(lane16), "s"(m0v), "s"(gsrc), "s"(z1)
                 : "memory", "scc");
}
__device__ __forceinline__ void mfma3z_dma2(f16v& c0, f16v& c1, const float4& a, const float4& b, unsigned lane16, unsigned m0a,
                                            const char* ga, unsigned m0b, const char* gb, int z1) {
    asm volatile("s_mov_b32 m0, %9\n\tv_mfma_f32_32x32x2_f32 %0, %3, %6, %0\n\tglobal_load_lds_dwordx4 %8, %10\n\t"
                 "s_mov_b32 m0, %11\n\ts_cmp_lg_u32 %13, 0\n\ts_cbranch_scc1 1f\n\t"
                 "v_mfma_f32_32x32x2_f32 %1, %2, %5, %1\n\tv_mfma_f32_32x32x2_f32 %1, %4, %7, %1\n"
                 "1:\n\tglobal_load_lds_dwordx4 %8, %12"
                 : "+a"(c0), "+a"(c1)
                 : "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.y), "v"(b.z), "v"(b.w), "v"(lane16), "s"(m0a), "s"(ga), "s"(m0b), "s"(gb), "s"(z1)
                 : "memory", "scc");
}

// A buffer descriptor over [base, base + bytes); the base is made formally wave-uniform (it is: kernel arguments and
// wave-uniform selects of them), or the compiler wraps every access in a waterfall loop.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* base, int bytes) {
    const unsigned long long b = reinterpret_cast<unsigned long long>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0, bytes, 0x00020000);
}

__device__ __forceinline__ int xcd_block(int bid, int n) { return (n % 8 == 0) ? (bid % 8) * (n / 8) + bid / 8 : bid; }

// DBG: wave 0 of every workgroup writes shader-clock stamps to stamps[64 * blockIdx.x ...]: entry, prologue done, loop done,
// end, then the end of every chunk (4 + chunk, chunk < 26) -- tools/wino_timeline.py; DBG 2 adds the end of each of the
// 16 MFMA groups of chunks 0 and 1 (30 + 16 * chunk + group) and, at 62, the issue of the very first MFMA --
// tools/wino_group_timeline.py.
// PARTS: 1 = the input is given in up to four channel parts (about 6 % more cycles per chunk: every patch row selects
// its part with scalar arithmetic), 0 = one tensor, 2 = ONE tensor of `cpart` channels read shift_s x shift_s times: channel
// block (a, b) (a, b < shift_s; block = a * shift_s + b = channel / cpart) is the same planes displaced by (3a, 3b) pixels --
// the S x S blocks of 3 x 3 taps of a 5 x 5 / 7 x 7 filter read the (halo-carrying) input where it lies, instead of a
// stack of shifted copies (MotionEnc, mcnet.py:36-47); cpart must be a multiple of 8 (a chunk never straddles blocks).
// pool_*: ypool is written into a plane of pool_h x pool_w with its origin at (pool_oy, pool_ox) -- the halo-carrying input
// of the next layer.  addx / y2: second full-resolution output y2 = y + fixed_unpooling(addx), addx [N, K, H/2, W/2]; with
// addx and no y2 the sum is written to y itself.  Compile-time (EPI: 0 none, 1 second output y2, 2 the sum goes to y): as
// run-time branches inside the 16-channel store loop they cost every layer 3,400 cycles of epilogue (tools/wino_timeline.py)
// (DecCnn's unpool + residual add, mcnet.py:234-236, in the epilogue of the Residual block's last convolution: a tile
// is exactly one unpooling cell).
// EPI 3: no second output, and a plane with an odd side (H or W odd; plain input and output planes, no pooled output): the tile
// grid is ceil(H / 2) x ceil(W / 2), row H and column W are the zero padding -- read as 0, never stored.  Row starts are then only
// 4-byte aligned and column W is the next row's first pixel in memory, so a patch row's middle pair is two 4-byte loads (the
// second out of range past column W - 1) and an output row two 4-byte stores (the second dropped past column W - 1).  A variant
// of its own, so that the even-plane instantiations keep their instruction streams (and their counted waits) exactly.
// SKIP (timeline builds only; results are then wrong): 1 no patch transform; 4 that and no patch loads; 2 that and no V
// writes; 5 that and no output stores.
template <int ACT, int DBG = 0, int SKIP = 0, int PARTS = 0, bool TALL = false, int EPI = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void conv3x3(const float* __restrict__ x, const float* __restrict__ x1, const float* __restrict__ x2,
             const float* __restrict__ x3, int cpart, const float* __restrict__ U, const float* __restrict__ bias,
             float* __restrict__ y, float* __restrict__ ypool, int N, int C, int K, int H, int W, int in_h, int in_w,
             int in_oy, int in_ox, int Kpad, int nchunks, int kblocks, long long* __restrict__ stamps, int pool_h, int pool_w,
             int pool_oy, int pool_ox, const float* __restrict__ addx, float* __restrict__ y2, int shift_s, int part_magic,
             int zero_tail, DivMagic dv) {
    long long t_entry = 0, t_pro = 0, t_loop = 0, r_entry = 0, t_p1 = 0, t_p2 = 0, t_p3 = 0, t_p4 = 0, t_p5 = 0, t_e1 = 0, t_e2 = 0;
    if (DBG) { t_entry = __builtin_readcyclecounter(); r_entry = __builtin_amdgcn_s_memrealtime(); }
    // Every kernel argument the prologue reads, demanded HERE: the compiler otherwise fetches the ~45 argument dwords in five or
    // six batches, each issued where its first value is needed and each waited for on its own -- six trips to the scalar cache in
    // series were most of the 1,360-1,800 cycles a workgroup spent before its first patch load (tools/wino_timeline.py, set-up).
    const unsigned grid_n = gridDim.x;
    asm volatile("" : : "s"(grid_n), "s"(x), "s"(U), "s"(bias), "s"(cpart), "s"(N), "s"(C), "s"(K), "s"(H), "s"(W), "s"(in_h), "s"(in_w), "s"(in_oy),
                 "s"(in_ox), "s"(Kpad), "s"(nchunks), "s"(kblocks), "s"(dv.m_tpi), "s"(dv.s_tpi), "s"(dv.m_tw), "s"(dv.s_tw), "s"(dv.m_kb),
                 "s"(dv.s_kb));
    if (PARTS == 1) asm volatile("" : : "s"(x1), "s"(x2), "s"(x3));
    if (PARTS == 2) asm volatile("" : : "s"(shift_s), "s"(part_magic), "s"(zero_tail));
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int WTM = TALL ? TTM : TM, WTN = TALL ? TTN : TN;                   // output channels x tiles per workgroup
    constexpr int WSTAGE = TALL ? TSTAGE_FLOATS : STAGE_FLOATS;
    constexpr int NP = TALL ? 1 : 2;                                                // patches per thread and chunk
    const int wm = TALL ? wave : (wave & 1), wn = TALL ? 0 : (wave >> 1);           // 2 x 2 waves, or 4 x 1
    // n / d for n < 2^31 as (n * m) >> (32 + s), m = ceil(2^(32 + s) / d), s = floor(log2 d) (one less for a power of two), both
    // from the host (wino_div_magic); m == 0 stands for d == 1.  The compiler's runtime division is ~40 vector instructions; four
    // of them (image and tile row of the patch role and of the epilogue role) were most of 1,800 cycles of set-up per workgroup.
    auto fdiv = [](unsigned n, unsigned m, unsigned sh) -> unsigned {
        const unsigned q = __umulhi(n, m) >> sh;
        return __builtin_expect(m != 0, 1) ? q : n;          // (a select, not a branch)
    };
    const int bid = xcd_block(blockIdx.x, (int)grid_n);
    const int tb = (int)__builtin_amdgcn_readfirstlane(fdiv((unsigned)bid, (unsigned)dv.m_kb, (unsigned)dv.s_kb)), kb = bid - tb * kblocks;
    constexpr bool RAGGED = EPI == 3, ADDX = EPI == 1 || EPI == 2;
    const int TH = RAGGED ? (H + 1) >> 1 : H >> 1, TW = RAGGED ? (W + 1) >> 1 : W >> 1;
    const int tiles_per_image = TH * TW;
    const int tiles_total = N * tiles_per_image;             // < 2^29 / 4
    const long long plane = (long long)H * W;             // output plane
    // The input plane is in_h x in_w with output pixel (0, 0) at (in_oy, in_ox), in_ox even: (H, W, 0, 0) for an ordinary
    // tensor, whose border is the zero padding; a tensor that carries its own halo (tai_conv_shift_stack) has
    // (H + 2, W + 4, 1, 2) and no padding is applied inside it.
    const long long plane_in = (long long)in_h * in_w;

    // ---- patch role: tile `lane` of this block, channel slots (kk, s0), (kk, s0 + 1) of every chunk (wave-uniform).
    // A patch row is x[yy][2tx-1 .. 2tx+2]: the two middle values are one aligned 8-byte load per lane (the wave's 64
    // tiles are consecutive, so the wave reads 512 contiguous bytes); the outer two are the neighbouring lanes' middle
    // values (a wave-wide DPP shift), except for lane 0 / lane 63, which fetch theirs with one extra 2-lane load.
    // 128 x 32 shape: ONE patch per thread.  Lanes 0-31 hold the 32 tiles for channel slot (kk 0, k-step `wave`), lanes
    // 32-63 the same tiles for (kk 1, k-step `wave`): channels 8*chunk + 2*wave and + 1.  The second channel's plane offset
    // is part of those lanes' byte offsets, so the scalar channel offset stays wave-uniform.
    const int pkk = TALL ? (lane >> 5) : (wave & 1), ps0 = TALL ? wave : (wave >> 1) * 2;
    const int l5 = lane & 31;
    const int pt = TALL ? tb * TTN + l5 : tb * TN + lane;
    const bool pvalid = pt < tiles_total;
    const int ptc = pvalid ? pt : 0;
    const int pimg = (int)fdiv((unsigned)ptc, (unsigned)dv.m_tpi, (unsigned)dv.s_tpi);
    const int prem = ptc - pimg * tiles_per_image;
    const int pty = (int)fdiv((unsigned)prem, (unsigned)dv.m_tw, (unsigned)dv.s_tw), ptx = prem - pty * TW;
    // Loads go through a buffer descriptor over the whole input: a lane whose offset is OUT_OF_RANGE gets 0.0f back
    // without touching memory, which is the zero padding (rows above/below the image, tiles past the end) for free,
    // and the per-chunk channel offset rides in the instruction's scalar offset: no vector address arithmetic at all.
    constexpr unsigned OUT_OF_RANGE = 0x80000000u;          // the tensor is < 2^31 bytes (checked by the launcher)
    // The input may be given in up to four parts of `cpart` channels each (the operands of a torch.cat along the
    // channels that is then never materialised); every part is a contiguous [N, cpart, H, W] tensor.
    const int part_bytes = (int)((long long)N * cpart * plane_in * 4);
    const __amdgpu_buffer_rsrc_t xrsrc0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, part_bytes, 0x00020000);
    const unsigned long long xb0 = reinterpret_cast<unsigned long long>(x);
    const unsigned long long xd1 = reinterpret_cast<unsigned long long>(x1) - xb0, xd2 = reinterpret_cast<unsigned long long>(x2) - xb0,
                             xd3 = reinterpret_cast<unsigned long long>(x3) - xb0;
    // Left / right outer values: the neighbouring lane's middle pair when that lane is the neighbouring tile of the same
    // tile row, else an own load (first / last tile of a row, lanes 0 / 63) -- or nothing, where the column is
    // outside the input plane (the zero padding).
    const bool left_in = pvalid && 2 * ptx - 1 + in_ox >= 0, right_in = pvalid && 2 * ptx + 2 + in_ox < in_w;
    // (128 x 32 shape: lanes 31 | 32 are not neighbours -- different channels -- so both ends of each half-wave load their own)
    const bool first_lane = TALL ? l5 == 0 : lane == 0, last_lane = TALL ? l5 == 31 : lane == 63;
    // (as lane masks: the lanes that KEEP their own outer value)
    const unsigned long long keep_left = __builtin_amdgcn_ballot_w64(!(pvalid && ptx > 0 && !(TALL && first_lane))),
                             keep_right = __builtin_amdgcn_ballot_w64(!(pvalid && ptx < TW - 1 && !(TALL && last_lane)));
    const bool left_own = left_in && (ptx == 0 || first_lane), right_own = right_in && (ptx == TW - 1 || last_lane);
    unsigned off_mid[4], off_left[4], off_right[4];     // byte offsets from the channel plane of image 0
    unsigned off_mid1[4];                               // RAGGED: the middle pair's second value (out of range at column W)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = 2 * pty - 1 + i + in_oy;
        const bool rowok = pvalid && yy >= 0 && yy < in_h;
        // (32-bit arithmetic: the launcher refuses tensors of 2^29 elements or more)
        off_mid[i] = rowok ? ((unsigned)(pimg * cpart + (TALL ? pkk : 0)) * (unsigned)plane_in + (unsigned)(yy * in_w + 2 * ptx + in_ox)) * 4u
                           : OUT_OF_RANGE;
        off_left[i] = (rowok && left_own) ? off_mid[i] - 4u : OUT_OF_RANGE;
        off_right[i] = (rowok && right_own) ? off_mid[i] + 8u : OUT_OF_RANGE;
        off_mid1[i] = (rowok && 2 * ptx + 1 < W) ? off_mid[i] + 4u : OUT_OF_RANGE;      // (RAGGED: in_w == W, in_ox == 0)
    }

    // The bias rides in the accumulators: transform position (1, 1) enters all four outputs of a tile with coefficient +1
    // (A^T m A: o00, o01, o10, o11 each contain + m[1][1]), so accumulator block 5 starts at the lane's 16 bias values instead
    // of zero and the epilogue has no bias loads, no wait for them and 64 adds fewer.  Register j of a lane's block is output
    // channel k_base + 8 (j / 4) + j % 4 + 4 (lane / 32) (the MFMA's D layout): four 16-byte loads, each its four consecutive
    // channels; channels past K read 0.0 (out of range, checked per dword).
    float bv[16];
    {
        const __amdgpu_buffer_rsrc_t brsrc = uniform_rsrc(bias, K * 4);
        const int k_base0 = kb * WTM + wm * 32;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const auto q4 = __builtin_amdgcn_raw_buffer_load_b128(brsrc, (lane >> 5) * 16, (k_base0 + 8 * jj) * 4, 0);
            const float4 q = __builtin_bit_cast(float4, q4);
            bv[4 * jj] = q.x; bv[4 * jj + 1] = q.y; bv[4 * jj + 2] = q.z; bv[4 * jj + 3] = q.w;
        }
    }
    // (PARTS != 2: only block 5 is initialised; every other block is WRITTEN by its first MFMA of chunk 0, which takes C = 0)
    constexpr bool ZERO_INIT = PARTS == 2;
    f16v acc[16];
    if constexpr (ZERO_INIT) {
#pragma unroll
        for (int f = 0; f < 16; ++f)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[f][j] = 0.f;
    }
    float2 dm[3][NP][4];                       // [buffer][patch][row] middle values, as loaded (buffer 2: prologue only)
    float2 dlr[3][NP][4];                      // outer values (left, right): own loads of row-end tiles and of lanes 0 / 63

    // PARTS == 2: the scalar offset of a chunk's channel block -- minus its first channel, plus its displacement -- is the
    // same for every row of the chunk: computed once per chunk (per row it cost 12 % of the kernel)
    auto displaced_base = [&](int ch) -> int {
        // block = chunk / (chunks per block) by a multiply and a shift (part_magic = 2^20 / (cpart / 8) + 1 from the host;
        // exact for chunk counts < 2^10), block row = block / shift_s likewise: scalar-ALU work only -- a compare chain here
        // became v_cndmask / v_readfirstlane between the MFMAs and cost 12 % of the kernel
        const int part = (ch * part_magic) >> 20;                                      // wave-uniform
        const int pa = shift_s == 2 ? (part >> 1) : ((part * 11) >> 5), pb = part - pa * shift_s;
        return (3 * pa * in_w + 3 * pb - part * cpart * (int)plane_in) * 4;
    };
    // PARTS == 1: which part a chunk's eight channels lie in, that part's buffer descriptor and the scalar offset of the chunk's
    // first channel inside it -- ONCE per chunk (parts are multiples of 8 channels: a chunk never straddles two).  Per patch row
    // (8-24 times per chunk, round 1-3) the selection was ~10 scalar instructions and two v_readfirstlane each, and the descriptors
    // it kept alive were spilled into vector-register lanes (20-35 v_readlane / v_writelane per chunk body).
    auto part_base = [&](int ch, __amdgpu_buffer_rsrc_t& xr, int& base) {
        const int c0 = ch * KC;
        const int part = (c0 >= cpart) + (c0 >= 2 * cpart) + (c0 >= 3 * cpart);              // wave-uniform
        // (masks, not a ?: chain over the four pointers: that becomes a lookup table in scratch memory)
        const unsigned long long xp = xb0 + (xd1 & (0ull - (unsigned long long)(part == 1))) +
                                      (xd2 & (0ull - (unsigned long long)(part == 2))) + (xd3 & (0ull - (unsigned long long)(part == 3)));
        xr = uniform_rsrc(reinterpret_cast<const void*>(xp), part_bytes);
        base = __builtin_amdgcn_readfirstlane((int)((long long)(c0 - part * cpart) * plane_in * 4));
    };
    // what: 0 = the row's three loads (middle pair, own left, own right), 1 = the middle pair only, 2 = the two outer loads only;
    // xr / dbase (PARTS == 1): the chunk's part_base
    auto load_patch_row = [&](auto buf_c, int ch, int p, int i, int dbase = 0, int what = 0, __amdgpu_buffer_rsrc_t xr = __amdgpu_buffer_rsrc_t()) {
        constexpr int buf = decltype(buf_c)::value;
        // (128 x 32 shape: the even channel of the wave's pair; lanes 32-63 read c + 1 through their byte offsets)
        const int c = TALL ? ch * KC + 2 * ps0 : ch * KC + 2 * (ps0 + p) + pkk;
        // a padded channel (c >= C) reads channel 0: its transformed weights are zero, any finite value will do
        const int cc = c < C ? c : 0;
        __amdgpu_buffer_rsrc_t xrsrc;
        int soff;
        if (PARTS == 2) {
            // displaced reads of one tensor (C = shift_s^2 * cpart is a multiple of 8: no padded channel)
            xrsrc = xrsrc0;
            soff = dbase + (int)((long long)c * plane_in * 4);
        } else if (PARTS) {
            // (C = parts x cpart is a multiple of 8: no padded channel; c - 8 ch is 0..7, wave-uniform)
            xrsrc = xr;
            soff = dbase + (c - ch * KC) * (int)plane_in * 4;
        } else {
            xrsrc = xrsrc0;
            soff = (int)((long long)cc * plane_in * 4);
        }
        // 128 x 32 shape, odd C: channel C - 1's partner in lanes 32-63 would be channel 0 of the NEXT image (times zero weights,
        // but 0 x NaN / Inf there would reach this image): those lanes go out of range and read 0.0
        unsigned past = 0;
        if constexpr (TALL && PARTS == 0) past = (c + 1 >= C && pkk) ? OUT_OF_RANGE : 0u;
        if (what != 2) {
            if constexpr (RAGGED) {
                dm[buf][p][i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, off_mid[i] | past, soff, 0));
                dm[buf][p][i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, off_mid1[i] | past, soff, 0));
            } else {
                dm[buf][p][i] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(xrsrc, off_mid[i] | past, soff, 0));
            }
        }
        // own outer values (first / last tile of a tile row, lanes 0 / 63); every other lane is out of range: no memory access
        if (what != 1) {
            dlr[buf][p][i].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, off_left[i] | past, soff, 0));
            dlr[buf][p][i].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrsrc, off_right[i] | past, soff, 0));
        }
    };

    // The chunk's transformed weights for this output-channel block: 32 runs of 1 KB, global -> LDS without registers,
    // run (wave + 4r) by this wave's r-th DMA.  Written as asm (inside the MFMA groups) so that the compiler's wait-count
    // pass does not see an LDS store it cannot disambiguate from the operand reads (it would wait vmcnt(0) before every
    // ds_read); completion is awaited by the counted s_waitcnt at the end of the chunk.  Dynamic LDS starts at address 0.
    const unsigned lane16 = lane * 16;
    // 128 x 32 shape: 32 rows [q][kk][h] of 128 channels x 4 floats = 64 runs of 1 KB; wave w takes half (w & 1) of rows
    // (w >> 1) + 2r, r = 0..15.
    const long long dma_step = TALL ? (long long)Kpad * 32 : (long long)Kpad * 64;       // 2 rows / 4 runs further, in bytes
    auto dma_src = [&](int ch) {
        if constexpr (TALL)
            return reinterpret_cast<const char*>(U + ((long long)ch * 32 * Kpad + (long long)(wave >> 1) * Kpad + kb * TTM + (wave & 1) * 64) * 4);
        else
            return reinterpret_cast<const char*>(U + ((long long)ch * 32 * Kpad + kb * TM) * 4 + (long long)wave * Kpad * 4);
    };
    auto dma_dst = [&](int stage, int r) {
        return TALL ? (unsigned)((stage * TSTAGE_FLOATS + ((wave >> 1) + 2 * r) * 512 + (wave & 1) * 256) * 4)
                    : (unsigned)((stage * STAGE_FLOATS + (wave + 4 * r) * 256) * 4);
    };
    auto dma_weights = [&](int ch, int stage) {                              // all 8 (16) at once (prologue)
        const char* ub = dma_src(ch);
#pragma unroll
        for (int r = 0; r < (TALL ? 16 : 8); ++r)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                         : : "s"(dma_dst(stage, r)), "v"(lane16), "s"(ub + r * dma_step) : "memory");
    };

    // B^T d B of one patch on register pairs: a patch row is (left, m.x, m.y, right) = an outer pair and a middle pair;
    // the row pass is 8 packed adds on those pairs, the column pass 2 packed adds per row with operand-half selects, and
    // what comes out are exactly the position pairs of the LDS operand order.
    typedef float v2f __attribute__((ext_vector_type(2)));
    v2f tmid[NP][4], tout[NP][4];              // row-transformed patches: (t[r][1], t[r][2]) and (t[r][0], t[r][3])
    float4 wv[8];                              // per position pair: (patch 0 pair, patch 1 pair), as written to LDS
    auto transform_rows = [&](auto buf_c, int p) {
        constexpr int buf = decltype(buf_c)::value;
        v2f mid[4], out[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 m = dm[buf][p][i];
            // lane l takes lane l-1's m.y as its left value and lane l+1's m.x as its right value, unless that lane is
            // not the neighbouring tile (first / last tile of a tile row): then it KEEPS its own outer load (0.0 where the
            // column is padding).  A select on the lane mask, not a multiply by 0.0: the neighbouring lane may hold another
            // image, and 0 x NaN / Inf there would reach this one.  Lane 0 has no lane to its left: the instruction leaves
            // its register alone, i.e. its own load; likewise lane 63 on the right.  (The VOP2 select takes its mask from
            // vcc only; the scalar move in front of it is free next to the vector work.)
            float left = dlr[buf][p][i].x, right = dlr[buf][p][i].y;
            asm("s_mov_b64 vcc, %2\n\tv_cndmask_b32_dpp %0, %1, %0, vcc wave_shr:1 row_mask:0xf bank_mask:0xf"
                : "+v"(left) : "v"(m.y), "s"(keep_left) : "vcc");
            asm("s_mov_b64 vcc, %2\n\tv_cndmask_b32_dpp %0, %1, %0, vcc wave_shl:1 row_mask:0xf bank_mask:0xf"
                : "+v"(right) : "v"(m.x), "s"(keep_right) : "vcc");
            mid[i] = v2f{m.x, m.y};
            out[i] = v2f{left, right};
        }
        tmid[p][0] = mid[0] - mid[2]; tout[p][0] = out[0] - out[2];
        tmid[p][1] = mid[1] + mid[2]; tout[p][1] = out[1] + out[2];
        tmid[p][2] = mid[2] - mid[1]; tout[p][2] = out[2] - out[1];
        tmid[p][3] = mid[1] - mid[3]; tout[p][3] = out[1] - out[3];
    };
    auto transform_cols = [&](int p) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v2f vo, vm;
            // (v0, v3) = (t0 - t2, t1 - t3): low = tout.lo - tmid.hi, high = tmid.lo - tout.hi
            asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(vo) : "v"(tout[p][r]), "v"(tmid[p][r]));
            // (v1, v2) = (t1 + t2, t2 - t1): low = tmid.lo + tmid.hi, high = tmid.hi - tmid.lo
            asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(vm) : "v"(tmid[p][r]));
            if (p == 0) { wv[2 * r].x = vo.x; wv[2 * r].y = vo.y; wv[2 * r + 1].x = vm.x; wv[2 * r + 1].y = vm.y; }
            else        { wv[2 * r].z = vo.x; wv[2 * r].w = vo.y; wv[2 * r + 1].z = vm.x; wv[2 * r + 1].w = vm.y; }
        }
    };
    // LDS byte addresses (dynamic LDS starts at address 0), ONE register per stage, every position pair an immediate offset;
    // kept opaque to the optimiser, which otherwise materialises every (stage, pair) address in a register of its own --
    // 16 of them here and 32 for the operand reads below (48 vector registers of address constants in the chunk loop).
    unsigned wbase[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        if constexpr (TALL)   // [q][kk][h = ps0 / 2][tile][sl = ps0 % 2][e 0..1], 8 bytes per lane
            wbase[st] = (unsigned)((st * TSTAGE_FLOATS + 16 * 2 * TTM * 4 + ((pkk * 2 + (ps0 >> 1)) * TTN + l5) * 4 + (ps0 & 1) * 2) * 4);
        else                  // [q][kk][h = ps0 / 2][tile][sl 0..1][e 0..1], 16 bytes per lane
            wbase[st] = (unsigned)((st * STAGE_FLOATS + 16 * 2 * TM * 4 + ((pkk * 2 + (ps0 >> 1)) * TN + lane) * 4) * 4);
        asm volatile("" : "+v"(wbase[st]));
    }
    auto write_v = [&](int stage, int q) {
        if constexpr (TALL) {                  // one patch, 8 bytes per lane; pair q is 4 * TTN * 4 floats further
            const v2f val = v2f{wv[q].x, wv[q].y};
            asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(wbase[stage]), "v"(val), "i"(q * 4 * TTN * 4 * 4) : "memory");
        } else {                               // two patches, 16 bytes per lane
            // as two 8-byte writes: a ds_write_b128 at this lane stride costs ~50 cycles of MFMA time, two ds_write_b64 ~19
            // (profiles/r01_notes.md item 12)
            const v2f lo = v2f{wv[q].x, wv[q].y}, hi = v2f{wv[q].z, wv[q].w};
            asm volatile("ds_write_b64 %0, %1 offset:%3\n\tds_write_b64 %0, %2 offset:%4"
                         : : "v"(wbase[stage]), "v"(lo), "v"(hi), "i"(q * 4 * TN * 4 * 4), "i"(q * 4 * TN * 4 * 4 + 8) : "memory");
        }
    };
    const std::integral_constant<int, 0> B0;
    const std::integral_constant<int, 1> B1;
    const int last = nchunks - 1;

    // ---- prologue: all loads of chunks 0, 1 and 2 start at once (chunk 0 into a third register buffer), so that the
    // first chunks of the loop find their patches already there; chunk 0 is transformed into LDS stage 0 here.
    const std::integral_constant<int, 2> B2;
    if (DBG == 1) { __builtin_amdgcn_sched_barrier(0); t_p1 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    // A workgroup's ~200 vector-memory instructions of the prologue go through the CU's one address unit at ~12 cycles each
    // (2,200-2,700 cycles for 52 per wave, whatever the lanes do: tools/wino_timeline.py).  Two of a patch row's three loads are
    // the OWN outer values of first / last tiles of a tile row and of lanes 0 / 63 -- and in a tensor whose tile rows are cut at
    // wave boundaries (every bi-TAI shape: 64, 32, 16, ... tiles per row) those columns lie outside the image for every lane of
    // the wave.  So: the prologue issues them only if some lane wants them (wave-uniform branch); the chunk loop keeps issuing
    // them unconditionally in the shadow of its MFMAs, where they cost nothing and a branch would split the loop body.
    const bool need_edge = __builtin_amdgcn_ballot_w64(left_own || right_own) != 0;
    const int ch1p = min(1, last);
    int db0 = PARTS == 2 ? displaced_base(0) : 0, db1 = PARTS == 2 ? displaced_base(ch1p) : 0;
    __amdgpu_buffer_rsrc_t xr0 = xrsrc0, xr1 = xrsrc0;
    if (PARTS == 1) { part_base(0, xr0, db0); part_base(ch1p, xr1, db1); }
    // (the outer values start as zeros, written BEFORE any load is in flight and made opaque; written in an else-branch of the
    // test below they sat behind s_waitcnt vmcnt(0) -- the block is formally reachable from the loads' block -- and the wave
    // waited out its first loads' latency before it issued the weight DMA)
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dlr[2][p][i] = make_float2(0.f, 0.f); dlr[1][p][i] = make_float2(0.f, 0.f);
            asm volatile("" : "+v"(dlr[2][p][i].x), "+v"(dlr[2][p][i].y), "+v"(dlr[1][p][i].x), "+v"(dlr[1][p][i].y));
        }
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) load_patch_row(B2, 0, p, i, db0, 1, xr0);
    if (need_edge) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < 4; ++i) { load_patch_row(B2, 0, p, i, db0, 2, xr0); load_patch_row(B1, ch1p, p, i, db1, 2, xr1); }
    }
    // Issue order is pinned (the scheduler may not move anything across these points): [bias, chunk 0's patches, chunk 1's outer
    // values] [weight DMA of chunk 0] [middle pairs of chunk 1's patches: one load per patch row].  The counted wait in front of
    // the barrier below relies on it (tests/test_wino_isa.py counts).
    __builtin_amdgcn_sched_barrier(0);
    dma_weights(0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) load_patch_row(B1, ch1p, p, i, db1, 1, xr1);
    __builtin_amdgcn_sched_barrier(0);
    // (chunk 2's patches are loaded by chunk 0 itself, between its first MFMA groups: issued here the compiler sinks them below
    // the barrier, in front of the first MFMA, whatever the scheduling barriers say)
    if (DBG == 1) { t_p2 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    // The accumulator writes of the initialisation (16 for the bias block; all 256 for the displaced-read layers, ~1,000
    // cycles) are pinned here: left alone the compiler sinks them to just before the first MFMA, behind the barrier.
    if constexpr (ZERO_INIT) {
#pragma unroll
        for (int f = 0; f < 16; ++f)
            if (f != 5) asm volatile("" : "+a"(acc[f]));
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[5][j] = bv[j];
    asm volatile("" : "+a"(acc[5]));
    if (DBG == 1) { __builtin_amdgcn_sched_barrier(0); t_p3 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    transform_rows(B2, 0);
    transform_cols(0);
    if constexpr (!TALL) {
        transform_rows(B2, 1);
        transform_cols(1);
    }
    if (DBG == 1) { __builtin_amdgcn_sched_barrier(0); asm volatile("" :: "v"(wv[0].x), "v"(wv[7].y)); t_p4 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
    for (int q = 0; q < 8; ++q) write_v(0, q);
    if (DBG == 1) { __builtin_amdgcn_sched_barrier(0); t_p5 = __builtin_readcyclecounter(); }
    // The weight DMA of chunk 0 (invisible to the compiler's wait counting) must have landed; the middle pairs of chunk 1's
    // patches, issued behind it (pinned above: one load per patch row), need not -- chunk 0 waits for them where it transforms them.
    // Round 3 loaded chunk 2's patches here too and waited for everything (vmcnt(0)); the compiler had sunk those 24 loads BELOW
    // the barrier, between it and the first MFMA: 1,300 cycles from the barrier to the first MFMA (tools/wino_group_timeline.py).
    __builtin_amdgcn_sched_barrier(0);
    // (the input pointers are operands of the barrier statements: x is `__restrict__`, and a statement that is not handed a
    // noalias pointer provably cannot write through it -- the optimiser then moves loads of x ACROSS it, e.g. chunk 0's loads of
    // chunk 3's patches out of the peeled chunk 0 into the loop below, and the counted waits no longer count what they assume)
    // (x1-x3 only where they are used: for a single input tensor the compiler does not keep them in registers but RE-LOADS them from
    // the kernel-argument segment in front of every such statement and waits for the scalar load -- 110-240 cycles per chunk on the
    // 128 x 32 shape, found as a 4 % regression of its chunk loop in tools/wino_timeline.py)
    // (RAGGED: two loads per middle pair)
    constexpr int MIDS = RAGGED ? 2 * NP * 4 : NP * 4;
    if constexpr (PARTS == 1) asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" : : "n"(MIDS), "s"(x), "s"(x1), "s"(x2), "s"(x3) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" : : "n"(MIDS), "s"(x) : "memory");
    __builtin_amdgcn_sched_barrier(0);

    if (DBG) t_pro = __builtin_readcyclecounter();
    // operand rows [kk = lane / 32][h = 0][row]: byte address of the lane's row in each stage, opaque (see wbase)
    typedef float vf4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const vf4 lds_f4;
    auto lds_read4 = [](unsigned addr) { const vf4 v = *reinterpret_cast<lds_f4*>(addr); return make_float4(v.x, v.y, v.z, v.w); };
    unsigned abase[2], bbase[2];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        abase[st] = (unsigned)((st * WSTAGE + ((lane >> 5) * 2 * WTM + wm * 32 + (lane & 31)) * 4) * 4);
        bbase[st] = (unsigned)((st * WSTAGE + 16 * 2 * WTM * 4 + ((lane >> 5) * 2 * WTN + wn * 32 + (lane & 31)) * 4) * 4);
        asm volatile("" : "+v"(abase[st]), "+v"(bbase[st]));
    }

    // One chunk: 64 MFMAs in 16 groups of 4 (half a position pair each: two accumulators x two k-steps).  The fp32 MFMA
    // runs on the vector ALU itself, so vector instructions of this wave do not hide under it and every MFMA -> VALU ->
    // MFMA switch costs a few cycles more: the vector filler is kept in one run after a group.  LDS and memory
    // instructions do hide, and go between the first and the other three MFMAs of a group (a handful per group: more
    // than one MFMA's worth stalls the next).  Per chunk: transform the patches of chunk ch+1 (register buffer `nb`,
    // loaded one and a half chunks ago) after groups 0-3, write them to the other LDS stage in groups 4-11, start the
    // patch loads of chunk ch+3 into `nb` in groups 8-15; the MFMAs of groups 4-11 carry the weight DMA of chunk ch+1.
    // first_c (chunk 0 only): the patches of chunk 2 go into the OTHER register buffer in groups 0-7 (0-3 for one patch per thread).
    auto chunk = [&](int ch, auto stage_c, auto nb_c, auto first_c) {
        constexpr int stage = decltype(stage_c)::value;
        constexpr bool FIRST = decltype(first_c)::value;
        const std::integral_constant<int, 1 - decltype(nb_c)::value> ob_c;       // the buffer that holds chunk ch + 2
        const int ch2 = min(ch + 2, last);
        int dbase2 = (FIRST && PARTS == 2) ? displaced_base(ch2) : 0;
        __amdgpu_buffer_rsrc_t xr2 = xrsrc0, xr3 = xrsrc0;
        const int ch1 = min(ch + 1, last), ch3 = min(ch + 3, last);   // past the end: harmless repeats, never read
        const char* ub = dma_src(ch1);
        int dbase3 = PARTS == 2 ? displaced_base(ch3) : 0;
        if (PARTS == 1) {
            part_base(ch3, xr3, dbase3);
            if (FIRST) part_base(ch2, xr2, dbase2);
        }
        // this chunk's channel block (a, b) of the displaced reads: last block row / column -> zero transform row / column 3
        int zr = 0, zc = 0;
        if (PARTS == 2) {
            const int part = (ch * part_magic) >> 20;
            const int pa = shift_s == 2 ? (part >> 1) : ((part * 11) >> 5), pb = part - pa * shift_s;
            // (zero_tail: the filter size is not a multiple of 3, i.e. the last block's third tap row / column IS zero)
            // pa == S - 1 as integer arithmetic (pa / (S - 1): S = 2 -> pa, S = 3 -> pa >> 1): a bool select here came out
            // as v_cndmask + v_readfirstlane between the MFMAs
            zr = __builtin_amdgcn_readfirstlane(zero_tail * (shift_s == 2 ? pa : (pa >> 1)));
            zc = __builtin_amdgcn_readfirstlane(zero_tail * (shift_s == 2 ? pb : (pb >> 1)));
        }
        float4 a[2], b[2];
        a[0] = lds_read4(abase[stage]);
        b[0] = lds_read4(bbase[stage]);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int g = j >> 1;                                                        // position pair
            const int f0 = 4 * (g >> 1) + (g & 1), f1 = 4 * (g >> 1) + 3 - (g & 1);      // (4r, 4r+3) or (4r+1, 4r+2)
            // (ZQ: this half-group holds the first MFMAs of the workgroup on its two accumulator blocks -- they take C = 0)
            constexpr bool ZINIT = FIRST && PARTS != 2;
            const bool ZQ = ZINIT && (j & 1) == 0;
            if (PARTS == 2 && j >= 12) mfma1z(acc[f0], a[j & 1], b[j & 1], zr);
            else if (ZINIT && (j & 1) == 0 && f0 != 5) mfma1<ZINIT>(acc[f0], a[j & 1], b[j & 1]);
            else mfma1(acc[f0], a[j & 1], b[j & 1]);
            __builtin_amdgcn_sched_barrier(0);
            if (DBG == 2 && ch == 0 && j == 0 && tid == 0) stamps[64 * (long long)blockIdx.x + 62] = __builtin_readcyclecounter();
            if (j < 15) {       // operands of the next group: pair (j+1)/2, k-step half (j+1)%2
                a[(j + 1) & 1] = lds_read4(abase[stage] + (unsigned)((((j + 1) >> 1) * 4 + ((j + 1) & 1)) * WTM * 4 * 4));
                b[(j + 1) & 1] = lds_read4(bbase[stage] + (unsigned)((((j + 1) >> 1) * 4 + ((j + 1) & 1)) * WTN * 4 * 4));
            }
            if (j >= 4 && j < 8 && (SKIP < 2 || SKIP == 4)) { write_v(stage ^ 1, 2 * (j - 4)); write_v(stage ^ 1, 2 * (j - 4) + 1); }
            if constexpr (FIRST) {
                if (j < NP * 4 && SKIP < 3) load_patch_row(ob_c, ch2, j >> 2, j & 3, dbase2, 0, xr2);
            }
            if constexpr (TALL) {               // one patch: its four rows in groups 12-15
                if (j >= 12 && SKIP < 3) load_patch_row(nb_c, ch3, 0, j - 12, dbase3, 0, xr3);
            } else {
                if (j >= 8 && SKIP < 3) load_patch_row(nb_c, ch3, (j - 8) >> 2, (j - 8) & 3, dbase3, 0, xr3);     // (SKIP 4: no loads either)
            }
            __builtin_amdgcn_sched_barrier(0);
            const bool outer = (g & 1) == 0;        // pair (4r, 4r + 3): its second position is transform column 3
            if (PARTS == 2 && (j >= 12 || (outer && (j < 4 || j >= 12)))) {
                if (j >= 12) mfma3z(acc[f0], acc[f1], a[j & 1], b[j & 1], zr, outer ? zc : 0);
                else mfma3z(acc[f0], acc[f1], a[j & 1], b[j & 1], 0, zc);
            } else if (j < 4 || j >= 12) {
                if (ZQ) mfma3<ZINIT>(acc[f0], acc[f1], a[j & 1], b[j & 1]);
                else mfma3(acc[f0], acc[f1], a[j & 1], b[j & 1]);
            } else if constexpr (TALL) {          // 16 weight DMAs per chunk: two per group
                if (PARTS == 2 && outer)
                    mfma3z_dma2(acc[f0], acc[f1], a[j & 1], b[j & 1], lane16, dma_dst(stage ^ 1, 2 * j - 8), ub + (2 * j - 8) * dma_step,
                                dma_dst(stage ^ 1, 2 * j - 7), ub + (2 * j - 7) * dma_step, zc);
                else if (ZQ)
                    mfma3_dma2<ZINIT>(acc[f0], acc[f1], a[j & 1], b[j & 1], lane16, dma_dst(stage ^ 1, 2 * j - 8), ub + (2 * j - 8) * dma_step,
                                      dma_dst(stage ^ 1, 2 * j - 7), ub + (2 * j - 7) * dma_step);
                else
                    mfma3_dma2(acc[f0], acc[f1], a[j & 1], b[j & 1], lane16, dma_dst(stage ^ 1, 2 * j - 8), ub + (2 * j - 8) * dma_step,
                               dma_dst(stage ^ 1, 2 * j - 7), ub + (2 * j - 7) * dma_step);
            } else if (PARTS == 2 && outer)
                mfma3z_dma(acc[f0], acc[f1], a[j & 1], b[j & 1], lane16, dma_dst(stage ^ 1, j - 4), ub + (j - 4) * dma_step, zc);
            else if (ZQ) mfma3_dma<ZINIT>(acc[f0], acc[f1], a[j & 1], b[j & 1], lane16, dma_dst(stage ^ 1, j - 4), ub + (j - 4) * dma_step);
            else mfma3_dma(acc[f0], acc[f1], a[j & 1], b[j & 1], lane16, dma_dst(stage ^ 1, j - 4), ub + (j - 4) * dma_step);
            __builtin_amdgcn_sched_barrier(0);
            if (SKIP < 1) {
                if (j == 0) transform_rows(nb_c, 0);
                if (j == 1) transform_cols(0);
                if (!TALL && j == 2) transform_rows(nb_c, 1);
                if (!TALL && j == 3) transform_cols(1);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (DBG == 2 && ch < 2 && tid == 0) stamps[64 * (long long)blockIdx.x + 30 + 16 * ch + j] = __builtin_readcyclecounter();
        }
        // the last weight DMA (group 11) is older than the 12 patch loads of groups 12-15: at most 12 outstanding <=>
        // the weights have landed (RAGGED: 16, four loads per patch row)
        if constexpr (RAGGED) {
            if constexpr (PARTS == 1) asm volatile("s_waitcnt vmcnt(16)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" : : "s"(x), "s"(x1), "s"(x2), "s"(x3) : "memory");
            else asm volatile("s_waitcnt vmcnt(16)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" : : "s"(x) : "memory");
        } else {
            if constexpr (PARTS == 1) asm volatile("s_waitcnt vmcnt(12)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" : : "s"(x), "s"(x1), "s"(x2), "s"(x3) : "memory");
            else asm volatile("s_waitcnt vmcnt(12)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" : : "s"(x) : "memory");
        }
        if (DBG && tid == 0 && ch < 26) stamps[64 * (long long)blockIdx.x + 4 + ch] = __builtin_readcyclecounter();
    };
    const std::integral_constant<bool, true> FIRST_CHUNK;
    const std::integral_constant<bool, false> LATER_CHUNK;
    chunk(0, B0, B1, FIRST_CHUNK);              // even chunk: LDS stage 0, consumes and refills register buffer 1
    for (int ch = 1; ch + 1 < nchunks; ch += 2) {
        chunk(ch, B1, B0, LATER_CHUNK);
        chunk(ch + 1, B0, B1, LATER_CHUNK);
    }
    if (!(nchunks & 1)) chunk(last, B1, B0, LATER_CHUNK);    // (a conditional second call inside the loop makes the allocator spill)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");     // last MFMA (16 passes) -> accumulator reads below
    if (DBG) t_loop = __builtin_readcyclecounter();

    // ---- inverse transform, bias, activation, store: lane holds (tile et, 16 output channels) x 16 positions.
    // Buffer addressing again: the output channel rides in the scalar offset, tiles past the end and channels past K
    // are out-of-range lanes (dropped by the hardware), so there is neither address arithmetic nor a branch per store.
    // (the lane id is taken afresh: kept live across the chunk loop, whose bodies use every vector register, it was spilled)
    int lane_e;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
    const int half = lane_e >> 5;
    const int et = tb * WTN + wn * 32 + (lane_e & 31);
    const bool evalid = et < tiles_total;
    const int etc = evalid ? et : 0;
    const int eimg = (int)fdiv((unsigned)etc, (unsigned)dv.m_tpi, (unsigned)dv.s_tpi);
    const int erem = etc - eimg * tiles_per_image;
    const int ety = (int)fdiv((unsigned)erem, (unsigned)dv.m_tw, (unsigned)dv.s_tw), etx = erem - ety * TW;
    const __amdgpu_buffer_rsrc_t yrsrc = uniform_rsrc(y, (int)((long long)N * K * plane * 4));
    const unsigned voff0 = evalid ? ((unsigned)(eimg * K + 4 * half) * (unsigned)plane + (unsigned)((2 * ety) * W + 2 * etx)) * 4u
                                  : OUT_OF_RANGE;
    // (RAGGED: the second row and the second column of the plane's last tile row / column are row H / column W: dropped)
    const unsigned voff1 = (evalid && (!RAGGED || 2 * ety + 1 < H)) ? voff0 + (unsigned)W * 4u : OUT_OF_RANGE;
    const bool col1 = !RAGGED || 2 * etx + 1 < W;
    const unsigned voff0r = (evalid && col1) ? voff0 + 4u : OUT_OF_RANGE, voff1r = (voff1 != OUT_OF_RANGE && col1) ? voff1 + 4u : OUT_OF_RANGE;
    // optional second output: the 2x2 max pool of the activated output (nn.MaxPool2d(2) of ContentEnc, mcnet.py:86-117).
    // A tile IS a pooling window, so the pooled value is the max of the lane's four outputs.
    const long long pplane = (long long)pool_h * pool_w;      // (TH x TW with the origin at (0, 0) for a plain pooled tensor)
    const __amdgpu_buffer_rsrc_t prsrc = uniform_rsrc(ypool ? ypool : y, ypool ? (int)((long long)N * K * pplane * 4) : 0);
    const unsigned poff = evalid ? ((unsigned)(eimg * K + 4 * half) * (unsigned)pplane + (unsigned)((ety + pool_oy) * pool_w + etx + pool_ox)) * 4u
                                 : OUT_OF_RANGE;
    // optional third output: y2 = y + fixed_unpooling(addx); the lane's tile is one unpooling cell, addx lands on its (0, 0) pixel
    const long long aplane = plane >> 2;
    const __amdgpu_buffer_rsrc_t arsrc = uniform_rsrc(ADDX ? addx : y, ADDX ? (int)((long long)N * K * aplane * 4) : 0);
    const __amdgpu_buffer_rsrc_t y2rsrc = uniform_rsrc(EPI == 1 ? y2 : y, EPI == 1 ? (int)((long long)N * K * plane * 4) : 0);
    const unsigned aoff = evalid ? ((unsigned)(eimg * K + 4 * half) * (unsigned)aplane + (unsigned)(ety * TW + etx)) * 4u : OUT_OF_RANGE;
    const int klim = K - 4 * half;                           // this lane's channel is k_lo + 4 * half
    const int k_base = kb * WTM + wm * 32;
    // the values to add (EPI): all 16 loads issued here, ahead of the inverse transform that hides their latency -- left inside
    // the store loop each one was waited for where it was used (SQ_WAIT_ANY 25-31 % of the wave cycles on these instances)
    float axv[16];
    if (ADDX) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k_lo = k_base + 8 * (j >> 2) + (j & 3);
            axv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(arsrc, k_lo < klim ? aoff : OUT_OF_RANGE, (int)((long long)k_lo * aplane * 4), 0));
        }
    }
    // A^T m A, one column of transform positions at a time, so that at most a few accumulator tuples are in vector registers at
    // once (copying all 256 accumulators out first makes the allocator shuffle registers for thousands of instructions), on
    // register PAIRS (two adjacent channels of a lane's 16): every add of the row pass and of the column pass's partial sums is
    // one v_pk_add_f32 -- the subtractions too, which the compiler leaves as two v_sub_f32 (192 of them in round 3's epilogue:
    // the fp32 MFMA shares the vector ALU, so every vector instruction here is MFMA time lost).  The LAST operation on each output
    // is scalar, so that its result can be written straight into the register pair the 8-byte store wants ((0,0) next to (0,1) of
    // ONE channel).  The four outputs are accumulated column by column -- same order of additions as t0[0] + t0[1] + t0[2] etc.
    v2f o00[8], o01[8], o10[8], o11[8];
    float r00v[16], r01v[16], r10v[16], r11v[16];
    auto pk_sub = [](v2f a, v2f b2) { v2f d; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b2)); return d; };
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const v2f m0 = v2f{acc[b][2 * q], acc[b][2 * q + 1]}, m1 = v2f{acc[4 + b][2 * q], acc[4 + b][2 * q + 1]},
                      m2 = v2f{acc[8 + b][2 * q], acc[8 + b][2 * q + 1]}, m3 = v2f{acc[12 + b][2 * q], acc[12 + b][2 * q + 1]};
            const v2f t0 = (m0 + m1) + m2;
            const v2f t1 = pk_sub(pk_sub(m1, m2), m3);
            if (b == 0) { o00[q] = t0; o10[q] = t1; }
            if (b == 1) { o00[q] = o00[q] + t0; o01[q] = t0; o10[q] = o10[q] + t1; o11[q] = t1; }
            if (b == 2) {
                r00v[2 * q] = o00[q].x + t0.x; r00v[2 * q + 1] = o00[q].y + t0.y;
                r10v[2 * q] = o10[q].x + t1.x; r10v[2 * q + 1] = o10[q].y + t1.y;
                o01[q] = pk_sub(o01[q], t0); o11[q] = pk_sub(o11[q], t1);
            }
            if (b == 3) {
                r01v[2 * q] = o01[q].x - t0.x; r01v[2 * q + 1] = o01[q].y - t0.y;
                r11v[2 * q] = o11[q].x - t1.x; r11v[2 * q + 1] = o11[q].y - t1.y;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (DBG == 1) { __builtin_amdgcn_sched_barrier(0); asm volatile("" :: "v"(r00v[0]), "v"(r11v[15])); t_e1 = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
    // ReLU as the bare instruction: fmaxf() comes with a canonicalising v_max_f32 x, x, x in front of it (IEEE mode: 108 extra
    // vector instructions in round 3's epilogue); the sums above are canonical already
    auto relu = [](float v) { asm("v_max_f32 %0, 0, %0" : "+v"(v)); return v; };
    typedef int v2i __attribute__((ext_vector_type(2)));
    // Store loop in two forms, chosen by a wave-uniform branch: every channel of the wave's 32 exists (every layer but K = 51) --
    // no per-channel masking of the store offsets (3-4 vector instructions per channel in round 3) -- or not.  The pooled second
    // output has a loop of its own behind ONE branch (inside the channel loop the branch was taken 16 times).
    auto store_all = [&](auto masked_c) {
        constexpr bool MASKED = decltype(masked_c)::value;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k_lo = k_base + 8 * (j >> 2) + (j & 3);
            float r00 = r00v[j], r01 = r01v[j], r10 = r10v[j], r11 = r11v[j];      // (the bias came in through accumulator block 5)
            if (ACT == 1) { r00 = relu(r00); r01 = relu(r01); r10 = relu(r10); r11 = relu(r11); }
            if (ACT == 2) { r00 = tanhf(r00); r01 = tanhf(r01); r10 = tanhf(r10); r11 = tanhf(r11); }
            const bool kok = MASKED ? k_lo < klim : true;
            const int soff = (int)((long long)k_lo * plane * 4);
            const float ax = ADDX ? axv[j] : 0.f;
            if (EPI == 2) r00 += ax;             // only the sum is wanted: it IS the output
            r00v[j] = r00; r01v[j] = r01; r10v[j] = r10; r11v[j] = r11;
            if (RAGGED) {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, r00), yrsrc, kok ? voff0 : OUT_OF_RANGE, soff, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, r01), yrsrc, kok ? voff0r : OUT_OF_RANGE, soff, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, r10), yrsrc, kok ? voff1 : OUT_OF_RANGE, soff, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, r11), yrsrc, kok ? voff1r : OUT_OF_RANGE, soff, 0);
            } else if (SKIP < 5 || r00 == 12345.f) {
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, make_float2(r00, r01)), yrsrc, kok ? voff0 : OUT_OF_RANGE, soff, 0);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, make_float2(r10, r11)), yrsrc, kok ? voff1 : OUT_OF_RANGE, soff, 0);
                if (EPI == 1) {
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, make_float2(r00 + ax, r01)), y2rsrc, kok ? voff0 : OUT_OF_RANGE, soff, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, make_float2(r10, r11)), y2rsrc, kok ? voff1 : OUT_OF_RANGE, soff, 0);
                }
            }
        }
        if (!RAGGED && ypool && SKIP < 5) {      // wave-uniform
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int k_lo = k_base + 8 * (j >> 2) + (j & 3);
                const bool kok = MASKED ? k_lo < klim : true;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, fmaxf(fmaxf(r00v[j], r01v[j]), fmaxf(r10v[j], r11v[j]))), prsrc,
                                                      kok ? poff : OUT_OF_RANGE, (int)((long long)k_lo * pplane * 4), 0);
            }
        }
    };
    if (k_base + 32 <= K) store_all(std::integral_constant<bool, false>());
    else store_all(std::integral_constant<bool, true>());
    if (DBG && tid == 0) {
        long long* st = stamps + 64 * (long long)blockIdx.x;
        st[0] = t_entry; st[1] = t_pro; st[2] = t_loop; st[3] = __builtin_readcyclecounter();
        if (DBG == 1) { st[40] = t_p1; st[41] = t_p2; st[42] = t_p3; st[43] = t_p4; st[44] = t_p5; st[45] = t_e1; }
        st[60] = r_entry; st[61] = __builtin_amdgcn_s_memrealtime();      // 100 MHz wall clock: shader clock = cycles / ticks x 100 MHz
    }
}

}  // namespace wino
