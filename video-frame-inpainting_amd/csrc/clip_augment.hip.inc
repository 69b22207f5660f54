// The clip pipeline's augmented way in (included by sepconv_capi.hip, after clip_pipeline.hip.inc whose tap / blend it shares through
// clip_taps.hip.inc): decoded uint8 RGB frames -> the fp32 [N, C, H + pad_h, W + pad_w] clip the models take, with a crop window, a
// top-bottom flip and a per-frame level table on top of what clip::from_frames does.  The definition is include/tai_sepconv.h's
// (tai_clip_from_frames_aug); tests/clip_augment_ref.py restates it in numpy and data._ClipReader.clip is the host path it equals bit
// for bit.
//
// Arithmetic contract, per output pixel (y, x) of frame n (source h x w, window {top, left, ch, cw} inside it, output H x W before
// padding) -- clip_pipeline.hip.inc's, word for word, with the WINDOW in the place of the source frame:
//   taps      src = (i + 0.5) * (n_in / n_out) - 0.5 in fp64 with n_in = ch (rows) or cw (columns), product and difference rounded
//             separately; i0 = floor(src); frac = src - i0; both taps clamped to [0, n_in - 1], i.e. to the window's edges: a pixel
//             outside the window never contributes.  Tap i of the window is source row top + i / source column left + i;
//   blend     clip::blend: fp64, every product and sum rounded on its own (contraction OFF), q = clip(floor(v + 0.5), 0, 255);
//   flips     output (y, x) reads resized (H - 1 - y if vflip, W - 1 - x if mirror): the flips follow the resize;
//   range     the fp32 value of level q is read from the frame's OWN [4][256] table, tables[index] -- the host computes it
//             (clip_pipeline.augment_level_tables: gamma, gain and offsets in float64, rounded once, then the host path's own torch
//             expressions), so photometric changes are exact by construction;
//   colour    C = 3: channel c of the output is source channel 2 - c (RGB -> BGR), value row 0[q];
//   gray      C = 1: (row 1[q_B] + row 2[q_G]) + row 3[q_R] in fp32: two rounded additions;
//   padding   rows >= H and columns >= W take level 0 of the NEUTRAL table `levels` (clip_pipeline.level_tables), never the frame's
//             own: -1.0 in colour, (row 1[0] + row 2[0]) + row 3[0] in gray, as clip::from_frames writes them.
//
// A frame's descriptor is DESC = 9 64-bit integers {byte offset into `frames`, h, w, flags (bit 0 = mirror, bit 1 = vflip), top, left,
// ch, cw, table index}.  The host side of the call validates the table it is given (call_refusal); the kernel re-checks each descriptor
// before it forms an address -- offset and sizes against frames_bytes, the window inside the frame, the table index below n_tables --
// and writes the padding level for every element of a frame whose descriptor fails.
//
// Layout: a workgroup owns (frame, band of output rows) and walks the items past GRID_CAP with a grid stride.  With per-frame tables
// the 4 KB a frame looks up no longer stay hot across the batch, so the workgroup stages the rows it needs in LDS once per item (row 0,
// 1 KB, for colour; rows 1-3, 3 KB, for gray; one 16-byte load per lane).  A lane owns one run of four output columns: its four
// column taps (two byte offsets and a fraction each) are computed once per item and reused for every row of the band it visits;
// `rw` lanes sit side by side on a row (all runs of the row when there are at most 256) and 256 / rw rows are in flight at once, so a
// wave's stores are contiguous (global_store_dwordx4; a row length that is no multiple of four or an unaligned output takes single
// words).  No atomics; every output element is written exactly once; a frame's bits depend on its descriptor, table and pixels only.

namespace clipaug {

constexpr int THREADS = 256;
constexpr int GRID_CAP = 2048;            // 8 workgroups per CU; the remaining (frame, band) items are walked with a grid stride
constexpr int DESC = 9;                   // int64 per frame
constexpr int ROWS_PER_LANE = 4;          // rows of a band one lane visits (full bands)

struct Geometry { int runs_per_row, rw, band_rows, bands; };

// runs of four columns per row; lanes side by side on a row; rows per band; bands per frame
inline Geometry geometry(long long Hp, long long Wp) {
    Geometry g;
    g.runs_per_row = (int)((Wp + 3) / 4);
    g.rw = g.runs_per_row < THREADS ? g.runs_per_row : THREADS;
    g.band_rows = (THREADS / g.rw) * ROWS_PER_LANE;
    g.bands = (int)((Hp + g.band_rows - 1) / g.band_rows);
    return g;
}

// one descriptor against the frame buffer and the table count: what the launcher asks of the host copy and the kernel of the device copy
__host__ __device__ __forceinline__ bool descriptor_ok(const long long* d, long long frames_bytes, int n_tables) {
    const long long off = d[0], h = d[1], w = d[2], top = d[4], left = d[5], ch = d[6], cw = d[7], tab = d[8];
    return off >= 0 && h > 0 && w > 0 && h < (1LL << 24) && w < (1LL << 24) && off <= frames_bytes && h * w * 3 <= frames_bytes - off &&
           top >= 0 && left >= 0 && ch >= 1 && cw >= 1 && ch <= h && cw <= w && top <= h - ch && left <= w - cw && tab >= 0 && tab < n_tables;
}

template <int C, bool VEC4>
__global__ __launch_bounds__(THREADS)
void from_frames_aug(const unsigned char* __restrict__ frames, long long frames_bytes, const long long* __restrict__ table,
                     const float* __restrict__ tables, int n_tables, const float* __restrict__ levels, float* __restrict__ out, int H, int W,
                     int Hp, int Wp, int runs_per_row, int rw, int band_rows, int bands, long long items) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float lut[4 * 256];
    const int tid = threadIdx.x;
    const int lane_run = tid % rw, lane_row = tid / rw, rp = THREADS / rw;           // lanes with lane_row >= rp have no row (256 % rw != 0)
    const long long plane = (long long)Hp * Wp;
    const float pad = C == 3 ? levels[0] : (levels[256] + levels[512]) + levels[768];
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int n = (int)(item / bands), band = (int)(item % bands);
        const long long* d = table + (long long)DESC * n;
        const bool frame_ok = descriptor_ok(d, frames_bytes, n_tables);
        const bool mirror = (d[3] & 1) != 0, vflip = (d[3] & 2) != 0;
        const int w = frame_ok ? (int)d[2] : 1, top = frame_ok ? (int)d[4] : 0, left = frame_ok ? (int)d[5] : 0;
        const int ch = frame_ok ? (int)d[6] : 1, cw = frame_ok ? (int)d[7] : 1;
        __syncthreads();                                    // the previous item's lookups are done
        if (frame_ok) {                                     // (uniform over the workgroup)
            const float4* src4 = reinterpret_cast<const float4*>(tables + (long long)d[8] * 1024);
            float4* lut4 = reinterpret_cast<float4*>(lut);
            if (C == 3) {
                if (tid < 64) lut4[tid] = src4[tid];
            } else {
                if (tid < 192) lut4[64 + tid] = src4[64 + tid];
            }
        }
        __syncthreads();
        if (lane_row >= rp) continue;                       // (rejoins at the barrier above)
        const unsigned char* src = frames + (frame_ok ? d[0] : 0);
        const int y_end = min((band + 1) * band_rows, Hp);
        for (int run0 = 0; run0 < runs_per_row; run0 += rw) {
            const int run = run0 + lane_run;
            if (run >= runs_per_row) break;
            int xa[4], xb[4];
            double fx[4];
            bool x_in[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                   // the lane's four column taps, once per item
                const int x = run * 4 + j;
                x_in[j] = frame_ok && x < W;
                xa[j] = xb[j] = 0;
                fx[j] = 0.0;
                if (x_in[j]) {
                    const clip::Tap tx = clip::tap(mirror ? W - 1 - x : x, W, cw);
                    xa[j] = (left + tx.i0) * 3;
                    xb[j] = (left + tx.i1) * 3;
                    fx[j] = tx.f;
                }
            }
            for (int y = band * band_rows + lane_row; y < y_end; y += rp) {
                const bool row_in = frame_ok && y < H;
                clip::Tap ty = {0, 0, 0.0};
                if (row_in) ty = clip::tap(vflip ? H - 1 - y : y, H, ch);
                const unsigned char* r0 = src + (long long)(top + ty.i0) * w * 3;
                const unsigned char* r1 = src + (long long)(top + ty.i1) * w * 3;
                float* o = out + (long long)n * C * plane + (long long)y * Wp + run * 4;
                if (C == 1) {
                    float g[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        g[j] = pad;
                        if (row_in && x_in[j]) {
                            const int qr = clip::blend(r0, r1, xa[j], xb[j], fx[j], ty.f);
                            const int qg = clip::blend(r0 + 1, r1 + 1, xa[j], xb[j], fx[j], ty.f);
                            const int qb = clip::blend(r0 + 2, r1 + 2, xa[j], xb[j], fx[j], ty.f);
                            g[j] = (lut[256 + qb] + lut[512 + qg]) + lut[768 + qr];
                        }
                    }
                    if (VEC4) {
                        *reinterpret_cast<float4*>(o) = make_float4(g[0], g[1], g[2], g[3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (run * 4 + j < Wp) o[j] = g[j];
                    }
                } else {
                    float v[3][4];                          // [output channel][column of the run]
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {       // output channel c = source channel 2 - c
                            v[c][j] = pad;
                            if (row_in && x_in[j]) v[c][j] = lut[clip::blend(r0 + (2 - c), r1 + (2 - c), xa[j], xb[j], fx[j], ty.f)];
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float* oc = o + c * plane;
                        if (VEC4) {
                            *reinterpret_cast<float4*>(oc) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (run * 4 + j < Wp) oc[j] = v[c][j];
                        }
                    }
                }
            }
        }
    }
}

// everything tai_clip_from_frames_aug refuses, before any runtime call; null: the launch goes ahead
inline const char* call_refusal(const unsigned char* frames, long long frames_bytes, const long long* table, const long long* table_host,
                                const float* tables, int n_tables, const float* levels, const float* out, int N, int c_dim, int H, int W,
                                int pad_h, int pad_w) {
    if (!frames || !table || !table_host || !tables || !levels || !out) return "clip_from_frames_aug: null pointer";
    if (c_dim != 1 && c_dim != 3) return "clip_from_frames_aug: c_dim must be 1 or 3";
    if (N <= 0 || H <= 0 || W <= 0 || pad_h < 0 || pad_w < 0 || frames_bytes <= 0 || n_tables <= 0)
        return "clip_from_frames_aug: needs N, H, W, frames_bytes, n_tables > 0 and pad_h, pad_w >= 0";
    const long long Hp = (long long)H + pad_h, Wp = (long long)W + pad_w;
    if (Hp >= (1LL << 24) || Wp >= (1LL << 24) || (long long)N * c_dim * Hp * Wp >= (1LL << 31) || frames_bytes >= (1LL << 40))
        return "clip_from_frames_aug: index space too large (2^31 output elements or more)";
    if (reinterpret_cast<uintptr_t>(tables) % 16 != 0) return "clip_from_frames_aug: the level tables must be 16-byte aligned";
    for (int n = 0; n < N; ++n) {
        const long long* d = table_host + (long long)DESC * n;
        const long long off = d[0], h = d[1], w = d[2], top = d[4], left = d[5], ch = d[6], cw = d[7], tab = d[8];
        if (h <= 0 || w <= 0 || h >= (1LL << 24) || w >= (1LL << 24))
            return "clip_from_frames_aug: a frame descriptor has a non-positive or oversized source size";
        if (off < 0 || off > frames_bytes || h * w * 3 > frames_bytes - off)
            return "clip_from_frames_aug: a frame descriptor points past the stated length of the frame buffer";
        if (ch < 1 || cw < 1) return "clip_from_frames_aug: a frame descriptor has a window with ch or cw < 1";
        if (top < 0 || left < 0 || ch > h || cw > w || top > h - ch || left > w - cw)
            return "clip_from_frames_aug: a frame descriptor has a window outside its frame";
        if (tab < 0 || tab >= n_tables) return "clip_from_frames_aug: a frame descriptor has a level-table index outside 0..n_tables-1";
    }
    return nullptr;
}

}  // namespace clipaug
