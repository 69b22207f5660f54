// Opt-in bf16 inference convolution (included by sepconv_capi.hip): k x k (k in {3, 5, 7}), stride 1, padding k / 2, as a direct
// implicit GEMM on v_mfma_f32_16x16x32_bf16.
//
//     y = act(bias + sum bf16_rne(x) * bf16_rne(w))      products exact, sums in fp32; x, y, bias fp32 in HBM
//
// GEMM view: M = output pixels, N = output channels, reduction = (input-channel chunk of KC = 16, tap).  One k-step of 32 is TWO taps
// of one chunk: lanes 0-31 of a fragment carry tap 2s (channels 0-7 / 8-15), lanes 32-63 tap 2s + 1; an odd k^2 pads the last step
// with a zero tap whose A lanes are zeroed in registers (never 0 x Inf).
//
// Workgroup: 256 threads = 4 waves; tile = MT = 64 MW pixels x NT = 64 output channels; wave w owns pixels [16 MW w, 16 MW (w + 1))
// and all 64 channels: MW x 4 accumulators of 16 x 16.  Per k-step a wave reads MW + 4 fragments (ds_read_b128) for 4 MW MFMAs.
//
// Pixels of a tile: IMG images x TH x TW (TH, TW even, chosen by the host from the plane: small planes put several images in one
// tile instead of wasting most of it), enumerated in 2 x 2 quads: pixel m = 4 q + 2 dy + dx.  The accumulator layout of the MFMA
// (row = 4 (lane >> 4) + reg) then gives every lane one whole quad of one channel, so the 2 x 2 max pool and the fixed unpooling
// (the quad's (0, 0) site) are lane-local epilogues.
//
// LDS, per chunk: the input patch (tile + halo k / 2 on every side, per image) as bf16, pixel-major with the 16 channels inner
// (32 bytes a pixel, so an A fragment of 8 channels is one ds_read_b128), staged once through registers (fp32 load ->
// v_cvt_pk_bf16_f32 -> ds_write_b128) and read for all k^2 taps; then the packed weights (tai_conv_bf16_pack_weights: the
// order the B fragments are read in, 1 KiB a fragment) in groups of G k-steps, copied as they lie.  Out-of-plane pixels, images
// past N and channels past C are staged as ZERO: a tile never reads another image's data, and a non-finite input reaches only
// the outputs whose window holds it.
//
// No split of the reduction and no atomics: each output sums chunk after chunk, tap pair after tap pair, in an order fixed by the
// layer's shape (C, k) alone, so repeated launches agree bit for bit and an image's output does not depend on its batch.

namespace cbf16 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KC = 16;                 // input channels per chunk
constexpr int NT = 64;                 // output channels per workgroup
constexpr int THREADS = 256;
constexpr int PIX_BYTES = KC * 2;      // one staged pixel: 16 bf16
constexpr int FRAG_BYTES = 64 * 16;    // one B fragment: 64 lanes x 8 bf16
constexpr int STEP_BYTES = 4 * FRAG_BYTES;     // the 4 fragments (64 output channels) of one k-step
constexpr int MAX_PATCH_BYTES = 32 * 1024;

__host__ __device__ constexpr int ksteps(int k) { return (k * k + 1) / 2; }
__host__ __device__ constexpr int group_steps(int k) { return k == 3 ? 5 : 7; }    // k-steps of weights staged at a time

struct Args {
    const float* x[4];        // input parts; part p holds channels [p cpart, (p + 1) cpart)
    int cpart;
    const uint4* w;           // packed weights
    const float* bias;
    float* y;                 // act(conv + bias), or the sum when addx is set and y2 is null
    float* ypool;             // optional 2 x 2 max pool of y
    const float* addx;        // optional: y2 = y + fixed_unpool(addx)
    float* y2;
    int N, C, K, H, W;
    int TH, TW, IMG, PH, PW, pitch;   // tile, patch and patch row pitch (pixels)
    int tiles_x, tiles_y, kblocks, nchunks;
};

__device__ __forceinline__ unsigned pack2(float a, float b) {      // v_cvt_pk_bf16_f32: round to nearest even, NaN kept
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

template <int ACT>
__device__ __forceinline__ float act(float v) {
    if (ACT == 1) return fmaxf(v, 0.f);
    if (ACT == 2) return tanhf(v);
    return v;
}

// Wp[kb][chunk][s][j][lane][e] (bf16) = w_conv[o][c][t / k][t % k] with o = 64 kb + 16 j + (lane & 15), t = 2 s + (lane >> 5),
// c = 16 chunk + 8 ((lane >> 4) & 1) + e; zero past K, C or k^2.  transposed: w is a ConvTranspose2d weight [C][K][k][k] and
// w_conv[o][c][ky][kx] = w[c][o][k - 1 - ky][k - 1 - kx].
__global__ __launch_bounds__(256)
void pack_weights(const float* __restrict__ w, unsigned* __restrict__ wp, int K, int C, int k, int transposed, int nchunks, long long pairs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pairs) return;
    const int e2 = (int)(i & 3);                    // element pair within the lane's 8
    const int lane = (int)((i >> 2) & 63);
    const int j = (int)((i >> 8) & 3);
    long long rest = i >> 10;
    const int S = (k * k + 1) / 2;
    const int s = (int)(rest % S);
    rest /= S;
    const int chunk = (int)(rest % nchunks);
    const int kb = (int)(rest / nchunks);
    const int o = kb * NT + j * 16 + (lane & 15);
    const int t = 2 * s + (lane >> 5);
    float v[2];
    for (int q = 0; q < 2; ++q) {
        const int c = chunk * KC + 8 * ((lane >> 4) & 1) + 2 * e2 + q;
        float x = 0.f;
        if (o < K && c < C && t < k * k) {
            const int ky = t / k, kx = t % k;
            x = transposed ? w[(((long long)c * K + o) * k + (k - 1 - ky)) * k + (k - 1 - kx)]
                           : w[(((long long)o * C + c) * k + ky) * k + kx];
        }
        v[q] = x;
    }
    wp[i] = pack2(v[0], v[1]);
}

template <int KS, int MW, int ACT>
__global__ __launch_bounds__(256)
void conv_bf16(Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int P = KS / 2;
    constexpr int S = ksteps(KS);
    constexpr int G = group_steps(KS);
    constexpr int MT = 64 * MW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 4, r = lane & 15;

    const int kb = blockIdx.x % a.kblocks;
    int tile = blockIdx.x / a.kblocks;
    const int tx = tile % a.tiles_x;
    tile /= a.tiles_x;
    const int ty = tile % a.tiles_y;
    const int ig = tile / a.tiles_y;
    const int x0 = tx * a.TW, y0 = ty * a.TH, n0 = ig * a.IMG;
    const int QW = a.TW >> 1, QH = a.TH >> 1;
    const int used = a.IMG * a.TH * a.TW;
    const int patch_px = a.IMG * a.PH * a.PW;
    unsigned char* const lds_w = lds + ((a.IMG * a.PH * a.pitch * PIX_BYTES + 15) & ~15);

    // byte address in the patch of each A row this lane reads (tap (0, 0)), plus the 16-byte half of the chunk's channels
    int abase[MW];
#pragma unroll
    for (int mf = 0; mf < MW; ++mf) {
        int m = wave * 16 * MW + mf * 16 + r;
        if (m >= used) m = 0;                   // rows past the tile's pixels: any staged pixel (never stored)
        const int q = m >> 2, sub = m & 3;
        const int qx = q % QW, qy = (q / QW) % QH, i = q / (QW * QH);
        abase[mf] = ((i * a.PH + 2 * qy + (sub >> 1)) * a.pitch + 2 * qx + (sub & 1)) * PIX_BYTES + (h & 1) * 16;
    }
    const int pitchB = a.pitch * PIX_BYTES;

    f32x4 acc[MW][4];
#pragma unroll
    for (int mf = 0; mf < MW; ++mf)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[mf][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const long long HW = (long long)a.H * a.W;
    const uint4* wsrc = a.w + (long long)kb * a.nchunks * S * (STEP_BYTES / 16);
    for (int ch = 0; ch < a.nchunks; ++ch) {
        __syncthreads();                        // the previous chunk's reads of the patch and the weights are done
        for (int px = tid; px < patch_px; px += THREADS) {
            const int i = px / (a.PH * a.PW), rem = px - i * (a.PH * a.PW);
            const int py = rem / a.PW, pxx = rem - py * a.PW;
            const int n = n0 + i, gy = y0 + py - P, gx = x0 + pxx - P;
            const bool in = n < a.N && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            float v[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int cg = ch * KC + c;
                float t = 0.f;
                if (in && cg < a.C) {
                    const int p = cg / a.cpart, cl = cg - p * a.cpart;
                    t = a.x[p][((long long)n * a.cpart + cl) * HW + (long long)gy * a.W + gx];
                }
                v[c] = t;
            }
            uint4* dst = reinterpret_cast<uint4*>(lds + ((i * a.PH + py) * a.pitch + pxx) * PIX_BYTES);
            dst[0] = uint4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
            dst[1] = uint4{pack2(v[8], v[9]), pack2(v[10], v[11]), pack2(v[12], v[13]), pack2(v[14], v[15])};
        }
#pragma unroll
        for (int s0 = 0; s0 < S; s0 += G) {
            const int gs = S - s0 < G ? S - s0 : G;
            if (s0 > 0) __syncthreads();        // the previous group's reads of the weights are done
            const uint4* src = wsrc + ((long long)ch * S + s0) * (STEP_BYTES / 16);
            for (int u = tid; u < gs * (STEP_BYTES / 16); u += THREADS)
                reinterpret_cast<uint4*>(lds_w)[u] = src[u];
            __syncthreads();
#pragma unroll
            for (int sl = 0; sl < G; ++sl) {
                const int s = s0 + sl;
                if (s < S) {
                    const int t0 = 2 * s, t1 = 2 * s + 1;
                    const bool pad = t1 >= KS * KS;
                    const int off = (h < 2) ? ((t0 / KS) * pitchB + (t0 % KS) * PIX_BYTES)
                                            : (pad ? 0 : (t1 / KS) * pitchB + (t1 % KS) * PIX_BYTES);
                    bf16x8 b[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        b[j] = *reinterpret_cast<const bf16x8*>(lds_w + (sl * 4 + j) * FRAG_BYTES + lane * 16);
#pragma unroll
                    for (int mf = 0; mf < MW; ++mf) {
                        bf16x8 av = *reinterpret_cast<const bf16x8*>(lds + abase[mf] + off);
                        if (pad && h >= 2) av = bf16x8{};      // the padding tap: zero operands, whatever is staged
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[mf][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b[j], acc[mf][j], 0, 0, 0);
                    }
                }
            }
        }
    }

    // epilogue: lane (h, r) of accumulator (mf, j) holds quad q = 4 (MW wave + mf) + h of output channel 64 kb + 16 j + r
    const bool even_w = (a.W & 1) == 0;
#pragma unroll
    for (int mf = 0; mf < MW; ++mf) {
        const int q = (wave * MW + mf) * 4 + h;
        if (q * 4 >= used) continue;
        const int qx = q % QW, qy = (q / QW) % QH, i = q / (QW * QH);
        const int n = n0 + i, oy = y0 + 2 * qy, ox = x0 + 2 * qx;
        if (n >= a.N || oy >= a.H || ox >= a.W) continue;
        const bool right = ox + 1 < a.W, below = oy + 1 < a.H;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = kb * NT + j * 16 + r;
            if (o >= a.K) continue;
            const float bo = a.bias[o];
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act<ACT>(acc[mf][j][e] + bo);
            const long long plane = ((long long)n * a.K + o) * HW;
            const long long at = plane + (long long)oy * a.W + ox;
            if (a.ypool)
                a.ypool[((long long)n * a.K + o) * (HW / 4) + (long long)(oy / 2) * (a.W / 2) + ox / 2] =
                    fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
            float s[4] = {v[0], v[1], v[2], v[3]};
            float* ys = a.y;
            if (a.addx) {
                s[0] = v[0] + a.addx[((long long)n * a.K + o) * (HW / 4) + (long long)(oy / 2) * (a.W / 2) + ox / 2];
                if (a.y2) {                     // both: y plain, y2 the sum
                    float* y2 = a.y2;
                    *reinterpret_cast<f32x2*>(y2 + at) = f32x2{s[0], s[1]};
                    *reinterpret_cast<f32x2*>(y2 + at + a.W) = f32x2{s[2], s[3]};
                } else {
                    v[0] = s[0];                // the sum only
                }
            }
            if (even_w) {
                *reinterpret_cast<f32x2*>(ys + at) = f32x2{v[0], v[1]};
                if (below) *reinterpret_cast<f32x2*>(ys + at + a.W) = f32x2{v[2], v[3]};
            } else {
                ys[at] = v[0];
                if (right) ys[at + 1] = v[1];
                if (below) {
                    ys[at + a.W] = v[2];
                    if (right) ys[at + a.W + 1] = v[3];
                }
            }
        }
    }
}

// The tile of a launch, from the plane alone: the even TH x TW and the image count IMG that need the fewest workgroups of MT pixels
// (ties: the fewest staged pixels), with the patch within MAX_PATCH_BYTES.  The row pitch of the patch is raised to 4 mod 8 pixels
// where that still fits: the four quads of a fragment then fall in distinct 16-byte slots of a 256-byte bank row for ds_read_b128.
// MT = 256 (MW = 4) where that grid fills the chip twice, else 128.
struct Plan { int MW, TH, TW, IMG, PH, PW, pitch, tiles_x, tiles_y, groups; long long blocks; int lds_bytes; };

inline Plan plan(int N, int K, int H, int W, int k) {
    const int P = k / 2, kblocks = (K + NT - 1) / NT;
    Plan best{};
    for (int MW = 4; MW >= 2; MW -= 2) {
        const int MT = 64 * MW;
        long long best_blocks = -1, best_staged = 0;
        const int wmax = ((W + 1) & ~1) < 32 ? ((W + 1) & ~1) : 32;
        const int hmax = ((H + 1) & ~1);
        for (int TW = 2; TW <= wmax; TW += 2)
            for (int TH = 2; TH <= hmax && TH * TW <= MT; TH += 2) {
                const int PH = TH + 2 * P, PW = TW + 2 * P;
                int IMG = MT / (TH * TW);
                if (IMG > N) IMG = N;
                while (IMG > 1 && IMG * PH * PW * PIX_BYTES > MAX_PATCH_BYTES) --IMG;
                if (IMG * PH * PW * PIX_BYTES > MAX_PATCH_BYTES) continue;
                const long long tiles = (long long)((N + IMG - 1) / IMG) * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
                const long long staged = tiles * IMG * PH * PW;
                if (best_blocks < 0 || tiles < best_blocks || (tiles == best_blocks && staged < best_staged)) {
                    best_blocks = tiles;
                    best_staged = staged;
                    best = Plan{MW, TH, TW, IMG, PH, PW, PW, (W + TW - 1) / TW, (H + TH - 1) / TH, (N + IMG - 1) / IMG,
                                tiles * kblocks, 0};
                }
            }
        if (MW == 4 && best.blocks >= 512) break;
    }
    int pitch = best.PW + ((12 - best.PW % 8) % 8);
    if (best.IMG * best.PH * pitch * PIX_BYTES <= MAX_PATCH_BYTES) best.pitch = pitch;
    best.lds_bytes = ((best.IMG * best.PH * best.pitch * PIX_BYTES + 15) & ~15) + group_steps(k) * STEP_BYTES;
    return best;
}

}  // namespace cbf16
