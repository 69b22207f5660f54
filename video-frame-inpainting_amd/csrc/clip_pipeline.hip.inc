// The clip pipeline's two ends (included by sepconv_capi.hip, after frame_metrics.hip.inc whose to_u8 it shares):
//   from_frames   decoded uint8 RGB frames [h_i, w_i, 3] -> the fp32 [N, C, H + pad_h, W + pad_w] clip the models take, with the
//                 arithmetic of video_frame_inpainting_amd/data.py (resize_bilinear, _ClipReader.clip) and util.py (fore_transform,
//                 bgr2gray), bit for bit;
//   to_uint8      fp32 [N, C, Hs, Ws] in [-1, 1] -> uint8 [N, h, w, C] pixels (util.frames_to_uint8 + crop + optional channel reversal).
//
// Arithmetic contract of from_frames, per output pixel (y, x) of frame n (source h x w, output H x W before padding):
//   taps      src = (i + 0.5) * (n_in / n_out) - 0.5 in fp64, product and difference rounded separately; i0 = floor(src); frac = src - i0;
//             both taps clamped to [0, n_in - 1] (numpy computes exactly this in resize_bilinear's `taps`);
//   blend     top = a * (1 - fx) + b * fx;  bot = c * (1 - fx) + d * fx;  v = top * (1 - fy) + bot * fy in fp64, every product and sum
//             rounded on its own: the whole file is compiled with contraction OFF -- one fused multiply-add here changes the rounding
//             of v and, at the .5 boundaries, the level;
//   level     q = clip(floor(v + 0.5), 0, 255);
//   mirror    output column x reads resized column W - 1 - x (the flip follows the resize on the host);
//   padding   rows >= H and columns >= W are level 0 in every channel (so -1.0 in colour and (0.114 L0 + 0.587 L0) + 0.2989 L0 =
//             -0.99990004 in gray, as the host's zero pad gives);
//   range     the fp32 value of level q is read from `levels`, a [4][256] table the HOST computes with the very torch expressions of the
//             host path: row 0 = (float(q) / 255) * 2 - 1, rows 1-3 = 0.1140 / 0.5870 / 0.2989 times row 0.  A true fp32 division is
//             what the host does; multiplying by a rounded 1/255 differs on 111 of the 256 levels, and the table is exact by construction;
//   colour    C = 3: channel c of the output is source channel 2 - c (RGB -> BGR);
//   gray      C = 1: (B' + G') + R' in fp32 with B' = row 1[q_B], G' = row 2[q_G], R' = row 3[q_R]: two rounded additions.
//
// Layout: one thread per run of four output columns of one output row, all channels; consecutive lanes own consecutive runs, so a
// wave writes 1 KiB of each output plane per store instruction (global_store_dwordx4; planes whose row length is not a multiple of
// four, or an unaligned output, take scalar stores).  The uint8 gathers of one output row touch two source rows, three bytes per tap;
// neighbouring lanes read neighbouring bytes of those rows, so the 64-byte lines they share are served by the vector L1 / L2 -- a frame
// is at most a few hundred KB and a batch tens of MB against a 4 MB L2 per XCD, and the kernel is launch- and latency-bound at these
// sizes, so the rows are NOT staged through LDS (that would add a barrier per row pair for no fewer HBM bytes).
//
// A frame's descriptor is four 64-bit integers {byte offset into `frames`, h, w, flags (bit 0 = mirror)}.  The host side of the call
// validates the table it is given; the kernel re-checks each descriptor against frames_bytes before it forms an address (a table that
// changed under a replayed graph must not become a wild read) and writes level 0 for a frame whose descriptor is out of range.

#include "clip_taps.hip.inc"          // clip::Tap, clip::tap, clip::blend: shared with clip_augment.hip.inc

namespace clip {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;          // 8 workgroups per CU; the rest of the index space is walked with a grid stride

template <int C, bool VEC4>
__global__ __launch_bounds__(THREADS)
void from_frames(const unsigned char* __restrict__ frames, long long frames_bytes, const long long* __restrict__ table,
                 const float* __restrict__ levels, float* __restrict__ out, int N, int H, int W, int Hp, int Wp, int runs_per_row,
                 long long total_runs) {
#pragma clang fp contract(off)
    const long long plane = (long long)Hp * Wp;
    for (long long idx = (long long)blockIdx.x * THREADS + threadIdx.x; idx < total_runs; idx += (long long)gridDim.x * THREADS) {
        const int run = (int)(idx % runs_per_row);
        const long long row = idx / runs_per_row;
        const int y = (int)(row % Hp);
        const int n = (int)(row / Hp);
        const long long off = table[4 * n], h64 = table[4 * n + 1], w64 = table[4 * n + 2];
        const bool mirror = (table[4 * n + 3] & 1) != 0;
        const bool frame_ok = off >= 0 && h64 > 0 && w64 > 0 && h64 < (1LL << 24) && w64 < (1LL << 24) &&
                              off <= frames_bytes && h64 * w64 * 3 <= frames_bytes - off;
        const int h = (int)h64, w = (int)w64;
        const unsigned char* src = frames + off;
        int q[4][3];                       // levels of the run's four pixels, source channel order (R, G, B)
        Tap ty = {0, 0, 0.0};
        const bool row_in = frame_ok && y < H;
        if (row_in) ty = tap(y, H, h);
        const unsigned char* r0 = src + (long long)ty.i0 * w * 3;
        const unsigned char* r1 = src + (long long)ty.i1 * w * 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = run * 4 + j;
            q[j][0] = q[j][1] = q[j][2] = 0;
            if (row_in && x < W) {
                const Tap tx = tap(mirror ? W - 1 - x : x, W, w);
#pragma unroll
                for (int c = 0; c < 3; ++c) q[j][c] = blend(r0 + c, r1 + c, tx.i0 * 3, tx.i1 * 3, tx.f, ty.f);
            }
        }
        float* o = out + (long long)n * C * plane + (long long)y * Wp + run * 4;
        if (C == 1) {
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = (levels[256 + q[j][2]] + levels[512 + q[j][1]]) + levels[768 + q[j][0]];
            if (VEC4) {
                *reinterpret_cast<float4*>(o) = make_float4(g[0], g[1], g[2], g[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (run * 4 + j < Wp) o[j] = g[j];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {                              // output channel c = source channel 2 - c
                float* oc = o + c * plane;
                if (VEC4) {
                    *reinterpret_cast<float4*>(oc) = make_float4(levels[q[0][2 - c]], levels[q[1][2 - c]], levels[q[2][2 - c]], levels[q[3][2 - c]]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (run * 4 + j < Wp) oc[j] = levels[q[j][2 - c]];
                }
            }
        }
    }
}

// One thread per output pixel: C bytes, channel-last.  The fp32 reads of a wave are 256 contiguous bytes per channel plane.
template <int C>
__global__ __launch_bounds__(THREADS)
void to_uint8(const float* __restrict__ x, unsigned char* __restrict__ out, int Hs, int Ws, int h, int w, int reverse, long long total) {
#pragma clang fp contract(off)
    const long long plane = (long long)Hs * Ws;
    for (long long idx = (long long)blockIdx.x * THREADS + threadIdx.x; idx < total; idx += (long long)gridDim.x * THREADS) {
        const int px = (int)(idx % w);
        const long long row = idx / w;
        const int py = (int)(row % h);
        const long long n = row / h;
        const float* p = x + n * C * plane + (long long)py * Ws + px;
        unsigned char* o = out + idx * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float unit;
            o[c] = (unsigned char)fmetrics::to_u8(p[(reverse ? C - 1 - c : c) * plane], unit);      // NaN -> 0 (fmaxf(NaN, -1) = -1)
        }
    }
}

inline unsigned blocks_for(long long items) {
    const long long b = (items + THREADS - 1) / THREADS;
    return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

}  // namespace clip
