// The way out of a PARTLY damaged frame (included by sepconv_capi.hip after frame_metrics.hip.inc, whose to_u8 it shares): the model's
// prediction where the damage is, the pipeline's own pixels everywhere else, and a linear ramp of `feather` pixels between them.  The
// definition is the one include/tai_sepconv.h writes down for tai_damage_composite and tests/damage_composite_ref.py restates in numpy;
// everything behind u() is integer arithmetic, so a frame has one correct bit pattern.
//   core     D(y, x) = 1 iff blocks[m][ty / bs][tx / bs] != 0 for some ty in {r0[y], r1[y]}, tx in {c0[x], c1[x]} (the source pixels the
//            bilinear resize reads with non-zero weight at model pixel (y, x); the host builds the four tap tables);
//   feather  R = feather + 1; A(y, x) = max(0, R - dist), dist = Chebyshev distance to the nearest D = 1 inside the h x w frame;
//   blend    out[y][x][c] = floor((2 (A P + (R - A) S) + R) / (2 R)), P = u(pred[c'][y][x]), S = u(src[c'][y][x]).
//
// Work split: a workgroup owns (item, tile of TILE_H x TILE_W pixels) and stages, in LDS,
//   1. core[TILE_H + 2 F][TILE_W + 2 F]: D on the tile and a halo of F = feather pixels (0 outside the frame), from the block map and the
//      tap tables' block indices of the staged rows and columns (two small int arrays, filled first);
//   2. rowd[TILE_H + 2 F][TILE_W]: per staged row the distance min |dx| <= F to a core pixel of that row, R where there is none;
//   3. alpha[TILE_H][TILE_W]: A = R - min over |dy| <= F of max(|dy|, rowd[y + dy][x]), floored at 0 -- the Chebyshev distance is separable;
// LDS at the largest feather: 62 * 94 + 62 * 64 + 32 * 64 bytes + 2 * (62 + 94) ints = 13,092 bytes.  Then every thread writes runs of 16
// output bytes of a tile row (a 16-byte store when the launcher found every row of `out` 16-byte aligned and w C a multiple of 16, single
// bytes otherwise); it reads pred only where A > 0 and src only where A < R.  What a frame gets depends on its own item alone: tiles only
// decide who computes a pixel.  The device copy of the item table is re-checked before an address is formed; a failed item's frame is
// left untouched.  The grid is capped at GRID_CAP workgroups; past it a workgroup strides.  No atomics.

namespace dcomp {

constexpr int THREADS = 256;
constexpr int TILE_H = 32, TILE_W = 64;
constexpr int MAX_FEATHER = 15;
constexpr int HALO_H = TILE_H + 2 * MAX_FEATHER, HALO_W = TILE_W + 2 * MAX_FEATHER;
constexpr long long GRID_CAP = 1LL << 12;
constexpr int ITEM_INTS = 4;                           // {pred offset, src offset, block map, output frame}

struct Args {
    const float* pred;
    const float* src;
    long long pred_elems, src_elems;
    const long long* table;        // device copy, [n_items][ITEM_INTS]
    long long n_items, n_maps, n_out;
    const unsigned char* blocks;   // [n_maps][Bh][Bw]
    const int* r0; const int* r1;  // [h]
    const int* c0; const int* c1;  // [w]
    unsigned char* out;            // [n_out][h][w][C]
    int Bh, Bw, bs, Hs, Ws, h, w, feather, reverse;
    int tiles_y, tiles_x;
    long long work;                // n_items * tiles_y * tiles_x
};

template <int C, bool VEC>
__global__ __launch_bounds__(THREADS)
void composite(const Args a) {
#pragma clang fp contract(off)
    __shared__ unsigned char core[HALO_H][HALO_W];
    __shared__ unsigned char rowd[HALO_H][TILE_W];
    __shared__ unsigned char alpha[TILE_H][TILE_W];
    __shared__ int rblk[2][HALO_H], cblk[2][HALO_W];
    const int t = threadIdx.x;
    const int F = a.feather, R = F + 1;
    const int sh = TILE_H + 2 * F, sw = TILE_W + 2 * F;                     // the staged region
    const long long plane = (long long)a.Hs * a.Ws, frame_elems = C * plane;
    const long long tiles = (long long)a.tiles_y * a.tiles_x;

    for (long long wi = blockIdx.x; wi < a.work; wi += gridDim.x) {
        const long long item = wi / tiles;
        const int tile = (int)(wi - item * tiles);
        const int y0 = tile / a.tiles_x * TILE_H, x0 = tile % a.tiles_x * TILE_W;
        const long long po = a.table[ITEM_INTS * item], so = a.table[ITEM_INTS * item + 1];
        const long long m = a.table[ITEM_INTS * item + 2], oi = a.table[ITEM_INTS * item + 3];
        const bool ok = po >= 0 && po <= a.pred_elems - frame_elems && so >= 0 && so <= a.src_elems - frame_elems &&
                        m >= 0 && m < a.n_maps && oi >= 0 && oi < a.n_out;
        if (!ok) continue;                                                   // uniform: the item is the workgroup's
        const unsigned char* map = a.blocks + m * a.Bh * a.Bw;

        // the block rows / columns the staged rows / columns read; -1: outside the frame, or a tap outside the map
        for (int i = t; i < sh + sw; i += THREADS) {
            const bool is_row = i < sh;
            const int p = is_row ? y0 - F + i : x0 - F + (i - sh);
            const int lim = is_row ? a.h : a.w, nblk = is_row ? a.Bh : a.Bw;
            int b0 = -1, b1 = -1;
            if (p >= 0 && p < lim) {
                const int t0 = is_row ? a.r0[p] : a.c0[p], t1 = is_row ? a.r1[p] : a.c1[p];
                if (t0 >= 0 && t0 / a.bs < nblk) b0 = t0 / a.bs;
                if (t1 >= 0 && t1 / a.bs < nblk) b1 = t1 / a.bs;
            }
            if (is_row) { rblk[0][i] = b0; rblk[1][i] = b1; } else { cblk[0][i - sh] = b0; cblk[1][i - sh] = b1; }
        }
        __syncthreads();
        for (int i = t; i < sh * sw; i += THREADS) {
            const int sy = i / sw, sx = i - sy * sw;
            const int ra = rblk[0][sy], rb = rblk[1][sy], ca = cblk[0][sx], cb = cblk[1][sx];
            unsigned d = 0u;
            if (ra >= 0 && ca >= 0) d |= map[ra * a.Bw + ca];
            if (ra >= 0 && cb >= 0 && cb != ca) d |= map[ra * a.Bw + cb];
            if (rb >= 0 && rb != ra) {
                if (ca >= 0) d |= map[rb * a.Bw + ca];
                if (cb >= 0 && cb != ca) d |= map[rb * a.Bw + cb];
            }
            core[sy][sx] = d ? 1 : 0;
        }
        __syncthreads();
        for (int i = t; i < sh * TILE_W; i += THREADS) {
            const int sy = i / TILE_W, x = i - sy * TILE_W;
            int best = R;
            for (int dx = -F; dx <= F; ++dx) {
                const int ad = dx < 0 ? -dx : dx;
                if (core[sy][x + F + dx] && ad < best) best = ad;
            }
            rowd[sy][x] = (unsigned char)best;
        }
        __syncthreads();
        for (int i = t; i < TILE_H * TILE_W; i += THREADS) {
            const int y = i / TILE_W, x = i - y * TILE_W;
            int best = R;
            for (int dy = -F; dy <= F; ++dy) {
                const int ad = dy < 0 ? -dy : dy, rd = rowd[y + F + dy][x];
                const int d = ad > rd ? ad : rd;
                if (d < best) best = d;
            }
            alpha[y][x] = (unsigned char)(R - best);
        }
        __syncthreads();

        const float* P = a.pred + po;
        const float* S = a.src + so;
        unsigned char* O = a.out + oi * a.h * a.w * C;
        constexpr int VECS_PER_ROW = TILE_W * C / 16;
        for (int i = t; i < TILE_H * VECS_PER_ROW; i += THREADS) {
            const int ty = i / VECS_PER_ROW, v = i - ty * VECS_PER_ROW;
            const int y = y0 + ty;
            if (y >= a.h) continue;
            unsigned char b[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int g = v * 16 + e, tx = g / C, c = g - tx * C, x = x0 + tx;
                b[e] = 0;
                if (x < a.w) {
                    const int A = alpha[ty][tx];
                    const long long at = (long long)(a.reverse ? C - 1 - c : c) * plane + (long long)y * a.Ws + x;
                    float unit;
                    const int p = A > 0 ? fmetrics::to_u8(P[at], unit) : 0;                       // NaN -> 0, as tai_frames_to_uint8
                    const int s = A < R ? fmetrics::to_u8(S[at], unit) : 0;
                    b[e] = (unsigned char)(A == R ? p : (A == 0 ? s : (2 * (A * p + (R - A) * s) + R) / (2 * R)));
                }
            }
            unsigned char* o = O + ((long long)y * a.w + x0) * C + v * 16;
            if (VEC) {
                if ((x0 * C + v * 16) < a.w * C) {                          // w C is a multiple of 16: a run is whole or absent
                    uint4 q;
                    q.x = b[0] | (b[1] << 8) | (b[2] << 16) | ((unsigned)b[3] << 24);
                    q.y = b[4] | (b[5] << 8) | (b[6] << 16) | ((unsigned)b[7] << 24);
                    q.z = b[8] | (b[9] << 8) | (b[10] << 16) | ((unsigned)b[11] << 24);
                    q.w = b[12] | (b[13] << 8) | (b[14] << 16) | ((unsigned)b[15] << 24);
                    *reinterpret_cast<uint4*>(o) = q;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    if (x0 * C + v * 16 + e < a.w * C) o[e] = b[e];
            }
        }
        __syncthreads();          // the tile's LDS is read before the next tile writes it
    }
}

// everything tai_damage_composite refuses, before any runtime call; null: the launch goes ahead
inline const char* refusal(const float* pred, long long pred_elems, const float* src, long long src_elems, const long long* table,
                           const long long* table_host, long long n_items, const unsigned char* blocks, long long n_maps, int Bh, int Bw,
                           int bs, const int* r0, const int* r1, const int* c0, const int* c1, const unsigned char* out, long long n_out,
                           int C, int Hs, int Ws, int h, int w, int feather) {
    if (!pred || !src || !table || !table_host || !blocks || !r0 || !r1 || !c0 || !c1 || !out) return "damage_composite: null pointer";
    if (C != 1 && C != 3) return "damage_composite: C must be 1 or 3";
    if (bs != 8 && bs != 16 && bs != 32) return "damage_composite: bs must be 8, 16 or 32";
    if (feather < 0 || feather > MAX_FEATHER) return "damage_composite: feather must be in 0..15";
    if (n_items < 1 || n_maps < 1 || n_out < 1 || Bh < 1 || Bw < 1) return "damage_composite: needs n_items, n_maps, n_out, Bh, Bw > 0";
    if (h < 1 || w < 1 || h > Hs || w > Ws) return "damage_composite: needs 0 < h <= Hs and 0 < w <= Ws";
    const long long frame_elems = (long long)C * Hs * Ws;
    if (frame_elems >= (1LL << 31) || n_items >= (1LL << 31) || n_out >= (1LL << 31) || n_maps * Bh * Bw >= (1LL << 31))
        return "damage_composite: index space too large (2^31 or more)";
    for (long long i = 0; i < n_items; ++i) {
        const long long* d = table_host + ITEM_INTS * i;
        if (d[0] < 0 || d[0] > pred_elems - frame_elems) return "damage_composite: an item's predicted frame lies outside pred_elems";
        if (d[1] < 0 || d[1] > src_elems - frame_elems) return "damage_composite: an item's source frame lies outside src_elems";
        if (d[2] < 0 || d[2] >= n_maps) return "damage_composite: an item's block map index is outside 0..n_maps-1";
        if (d[3] < 0 || d[3] >= n_out) return "damage_composite: an item's output frame index is outside 0..n_out-1";
    }
    return nullptr;
}

}  // namespace dcomp
