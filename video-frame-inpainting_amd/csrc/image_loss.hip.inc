// Pointwise (L2 / L1 / Charbonnier) + gradient-difference image loss and its gradient for up to three predictions against one ground
// truth, in one launch (included by sepconv_capi.hip); the definition is the one include/tai_sepconv.h writes down for tai_image_loss and
// tests/image_loss_ref.py restates in numpy:
//   x = (pred + 1) / 2, y = (gt + 1) / 2, d = x - y in fp32 (util.inverse_transform), NOT clipped; every fp32 operation as written;
//   rho(d) = d * d | |d| | sqrt(d * d + eps * eps);   rho'(d) = 2 * d | sgn(d) | d / sqrt(d * d + eps * eps);
//   gw(r, c) = (x[r,c] - x[r,c+1]) - (y[r,c] - y[r,c+1]) for r >= 1, c <= W-2;  gh(r, c) = (x[r,c] - x[r-1,c]) - (y[r,c] - y[r-1,c]) for
//   r >= 1, c >= 1 (losses.GDL's operand order);  sums of rho and of |gw| + |gh| in float64;
//   grad = fp32((double)rho'(d) * cp + S * cg), S = sgn(gw(r,c)) - sgn(gw(r,c-1)) + sgn(gh(r,c)) - sgn(gh(r+1,c)), each where it exists.
//
// Exactness: a pixel's gradient is a fixed expression of the pixel, its four neighbours and (cp, cg), with contraction off: it does not
// depend on the tiling, the other planes, npred or the other predictions.  Only the order of the two float64 sums belongs to the kernel
// (a lane's four pixels left to right, a butterfly over the wave, waves in order, tiles in order, planes in a fixed tree).  No atomics.
//
// Work split: one workgroup per (plane, 16 x 64 tile), 256 lanes, a lane owns four consecutive pixels of one row: one 16-byte load per
// array and one 16-byte store per gradient where the row's address allows (the row is inside the plane for all four and the address is a
// multiple of 16: planes with odd H * W alternate), single words otherwise.  The lane keeps its pixels in registers and shares them through
// LDS (row stride 72 words, the tile at column 4 so that a lane's four words are one aligned 16-byte slot); the one-pixel frame around
// the tile (top, bottom, left, right; no corners: no term reaches them) is loaded by the first 160 lanes.  A term belongs to the pixel
// (r, c) it is written for above, so every term is summed once.  LDS: 4 x 18 x 72 x 4 + 192 = 20,928 bytes.  The grid is capped at
// GRID_CAP workgroups; past it a workgroup strides over the tiles.

#include "loss_common.hip.inc"

namespace imgloss {

constexpr int TH = 16, TW = 64;            // pixels per tile
constexpr int THREADS = 256;               // TH rows x (TW / 4) lanes
constexpr int LW = TW + 8;                 // LDS row: 3 unused words, the left frame at 3, the tile at 4..67, the right frame at 68
constexpr int LH = TH + 2;                 // the top frame at row 0, the tile at 1..TH, the bottom frame at TH + 1
constexpr int MAXP = 3;
constexpr long long GRID_CAP = 1LL << 20;

struct Args {
    const float* pred[MAXP];
    float* grad[MAXP];                     // any may be null
    const float* gt;
    double* part;                          // [npred][planes * tiles][2]
    int npred, kind, H, W, nby, nbx;
    long long tiles_total;                 // planes * nby * nbx
    float e2;                              // eps * eps in fp32
    double cp, cg;
};

using namespace losscommon;

// the lane's four pixels of one array: registers and LDS; zero outside the plane (no term that exists reads those)
__device__ __forceinline__ void stage_row(const float* __restrict__ plane, float* __restrict__ s, int r, int c, int H, int W, int ty, int tx,
                                          float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (r < H && c < W) {
        const float* q = plane + (long long)r * W + c;
        if (c + 3 < W && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
            const float4 t = *reinterpret_cast<const float4*>(q);
            v[0] = range_map(t.x); v[1] = range_map(t.y); v[2] = range_map(t.z); v[3] = range_map(t.w);
        } else {
            // an empty statement the compiler cannot see through: without it the first word's load is hoisted out of both branches
            // and the 16-byte load above becomes a 4-byte and a 12-byte one
            asm volatile("" : "+v"(q));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < W) v[j] = range_map(q[j]);
        }
    }
    *reinterpret_cast<float4*>(s + (ty + 1) * LW + 4 + 4 * tx) = make_float4(v[0], v[1], v[2], v[3]);
}

// the frame: lanes 0..63 the row above, 64..127 the row below, 128..143 the column left, 144..159 the column right
__device__ __forceinline__ void stage_frame(const float* __restrict__ plane, float* __restrict__ s, int r0, int c0, int H, int W, int t) {
    int lr, lc;
    if (t < TW) { lr = 0; lc = 4 + t; }
    else if (t < 2 * TW) { lr = LH - 1; lc = 4 + t - TW; }
    else if (t < 2 * TW + TH) { lr = 1 + t - 2 * TW; lc = 3; }
    else { lr = 1 + t - 2 * TW - TH; lc = 4 + TW; }
    const int r = r0 - 1 + lr, c = c0 - 4 + lc;
    float v = 0.f;
    if (r >= 0 && r < H && c >= 0 && c < W) v = range_map(plane[(long long)r * W + c]);
    s[lr * LW + lc] = v;
}

__global__ __launch_bounds__(THREADS)
void tile_loss_grad(const Args a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float sy[LH * LW];
    __shared__ __attribute__((aligned(16))) float sx[MAXP][LH * LW];
    __shared__ double red[MAXP][2][THREADS / 64];
    const int H = a.H, W = a.W, npred = a.npred;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long plane_elems = (long long)H * W;
    const int tiles_per_plane = a.nby * a.nbx;

    for (long long tile = blockIdx.x; tile < a.tiles_total; tile += gridDim.x) {
        const long long plane = tile / tiles_per_plane;
        const int within = (int)(tile - plane * tiles_per_plane);
        const int by = within / a.nbx, bx = within - by * a.nbx;
        const int r0 = by * TH, c0 = bx * TW;
        const int r = r0 + ty, c = c0 + 4 * tx;
        const long long base = plane * plane_elems;

        float y[4], x[MAXP][4];
        stage_row(a.gt + base, sy, r, c, H, W, ty, tx, y);
#pragma unroll
        for (int i = 0; i < MAXP; ++i)
            if (i < npred) stage_row(a.pred[i] + base, sx[i], r, c, H, W, ty, tx, x[i]);
        if (threadIdx.x < 2 * TW + 2 * TH) {
            stage_frame(a.gt + base, sy, r0, c0, H, W, threadIdx.x);
#pragma unroll
            for (int i = 0; i < MAXP; ++i)
                if (i < npred) stage_frame(a.pred[i] + base, sx[i], r0, c0, H, W, threadIdx.x);
        }
        __syncthreads();

        const int lrow = (ty + 1) * LW + 4 + 4 * tx;
        const float4 yu = *reinterpret_cast<const float4*>(sy + lrow - LW), yd = *reinterpret_cast<const float4*>(sy + lrow + LW);
        const float yy[6] = {sy[lrow - 1], y[0], y[1], y[2], y[3], sy[lrow + 4]};
        const float yup[4] = {yu.x, yu.y, yu.z, yu.w}, ydn[4] = {yd.x, yd.y, yd.z, yd.w};
        const bool row_in = r < H, has_up = r >= 1, has_down = r <= H - 2;

#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            if (i >= npred) continue;
            const float4 xu = *reinterpret_cast<const float4*>(sx[i] + lrow - LW), xd = *reinterpret_cast<const float4*>(sx[i] + lrow + LW);
            const float xx[6] = {sx[i][lrow - 1], x[i][0], x[i][1], x[i][2], x[i][3], sx[i][lrow + 4]};
            const float xup[4] = {xu.x, xu.y, xu.z, xu.w}, xdn[4] = {xd.x, xd.y, xd.z, xd.w};
            double point = 0.0, gdl = 0.0;
            float g[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cc = c + j;
                if (!row_in || cc >= W) continue;
                const float xc = xx[j + 1], yc = yy[j + 1];
                const float d = xc - yc;
                float rho, drho;
                rho_drho(a.kind, d, a.e2, rho, drho);
                point = point + (double)rho;
                const bool left = cc >= 1, right = cc <= W - 2;
                const float gw = (xc - xx[j + 2]) - (yc - yy[j + 2]);          // gw(r, c)
                const float gwl = (xx[j] - xc) - (yy[j] - yc);                // gw(r, c - 1)
                const float gh = (xc - xup[j]) - (yc - yup[j]);               // gh(r, c)
                const float ghd = (xdn[j] - xc) - (ydn[j] - yc);              // gh(r + 1, c)
                const bool m1 = has_up && right, m2 = has_up && left, m3 = m2, m4 = has_down && left;
                if (m1) gdl = gdl + (double)__builtin_fabsf(gw);
                if (m3) gdl = gdl + (double)__builtin_fabsf(gh);
                const float t1 = m1 ? sgn(gw) : 0.f, t2 = m2 ? sgn(gwl) : 0.f, t3 = m3 ? sgn(gh) : 0.f, t4 = m4 ? sgn(ghd) : 0.f;
                const float S = ((t1 - t2) + t3) - t4;
                const double pa = (double)drho * a.cp, pb = (double)S * a.cg;
                g[j] = (float)(pa + pb);
            }
            float* gp = a.grad[i];
            if (gp != nullptr && row_in && c < W) {
                float* q = gp + base + (long long)r * W + c;
                if (c + 3 < W && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
                    *reinterpret_cast<float4*>(q) = make_float4(g[0], g[1], g[2], g[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (c + j < W) q[j] = g[j];
                }
            }
            point = wave_sum(point);
            gdl = wave_sum(gdl);
            if ((threadIdx.x & 63) == 0) {
                red[i][0][threadIdx.x >> 6] = point;
                red[i][1][threadIdx.x >> 6] = gdl;
            }
        }
        __syncthreads();          // (also: every read of sx / sy of this tile is done)
        if ((int)threadIdx.x < 2 * npred) {
            const int i = threadIdx.x >> 1, term = threadIdx.x & 1;
            double t = 0.0;
            for (int w = 0; w < THREADS / 64; ++w) t += red[i][term][w];
            a.part[((long long)i * a.tiles_total + tile) * 2 + term] = t;
        }
        // red is written again only after the next tile's first barrier, which this lane reaches after the reads above
    }
}

// One thread per (prediction, plane): its tiles in order.
__global__ __launch_bounds__(THREADS)
void finish_planes(const double* __restrict__ part, double* __restrict__ plane_terms, long long rows, int tiles) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // i * planes + plane
    if (n >= rows) return;
    const double* q = part + n * tiles * 2;
    double p = 0.0, g = 0.0;
    for (int t = 0; t < tiles; ++t) {
        p += q[2 * t];
        g += q[2 * t + 1];
    }
    plane_terms[2 * n] = p;
    plane_terms[2 * n + 1] = g;
}

// One workgroup per prediction: lane t sums the planes t, t + 256, ... in order, then a fixed halving tree; a function of the plane
// count alone.
__global__ __launch_bounds__(THREADS)
void finish_total(const double* __restrict__ plane_terms, double* __restrict__ totals, long long planes, double n_point, double n_gdl) {
#pragma clang fp contract(off)
    __shared__ double acc[2][THREADS];
    const double* q = plane_terms + (long long)blockIdx.x * planes * 2;
    double p = 0.0, g = 0.0;
    for (long long n = threadIdx.x; n < planes; n += THREADS) {
        p += q[2 * n];
        g += q[2 * n + 1];
    }
    acc[0][threadIdx.x] = p;
    acc[1][threadIdx.x] = g;
    __syncthreads();
    for (int h = THREADS / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            acc[0][threadIdx.x] = acc[0][threadIdx.x] + acc[0][threadIdx.x + h];
            acc[1][threadIdx.x] = acc[1][threadIdx.x] + acc[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double point = acc[0][0] / n_point, gdl = acc[1][0] / n_gdl;
        double* out = totals + 3 * blockIdx.x;
        out[0] = point;
        out[1] = gdl;
        out[2] = point + gdl;
    }
}

struct Plan {
    int nby, nbx;
    long long tiles_total;    // planes * nby * nbx
};

inline Plan plan(long long planes, int H, int W) {
    Plan p;
    p.nby = (H + TH - 1) / TH;
    p.nbx = (W + TW - 1) / TW;
    p.tiles_total = planes * p.nby * p.nbx;
    return p;
}

// what tai_image_loss and its workspace query refuse for the dimensions; null: they are taken
inline const char* refusal(int npred, long long planes, int H, int W) {
    if (npred < 1 || npred > MAXP) return "image_loss: npred must be 1, 2 or 3";
    if (planes < 1) return "image_loss: needs at least one plane";
    if (H < 2 || W < 2) return "image_loss: needs H, W >= 2 (the gradient-difference term)";
    const long long hw = (long long)H * W;
    if (hw >= (1LL << 31) || planes > ((1LL << 40) - 1) / hw) return "image_loss: tensor too large (planes H W >= 2^40 or H W >= 2^31)";
    if (plan(planes, H, W).tiles_total >= (1LL << 31)) return "image_loss: too many tiles (2^31 or more)";
    return nullptr;
}

}  // namespace imgloss
