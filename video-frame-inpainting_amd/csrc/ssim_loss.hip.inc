// Structural-similarity training loss and its gradient in one launch (included by sepconv_capi.hip); the definition is the one
// include/tai_sepconv.h writes down for tai_ssim_loss and tests/ssim_loss_ref.py restates in numpy:
//   x = (pred + 1) / 2, y = (gt + 1) / 2 in fp32 (util.inverse_transform), NOT clipped, then float64 for everything below;
//   7x7 uniform window over the (H-6) x (W-6) interior, L = 1, C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, covariance scaled by 49/48;
//   every 7x7 sum is a vertical 7-row sum (k = 0..6, from 0.0) followed by a horizontal sum of 7 of those (k = 0..6, from 0.0);
//   loss = 1 - mean over planes of (mean over the interior of S);  grad = d loss / d pred, rounded to fp32 once.
//
// Why float64: E[x^2] - E[x]^2 cancels against C2 = 9e-4; in fp32 the same expressions are off by 2e-4 in S on smooth planes.
//
// Exactness: a pixel's gradient and a window's S are fixed-order float64 expressions of the pixels around them with contraction off, so
// they do not depend on the tiling, the other planes or the launch; only the interior mean's summation order belongs to the kernel (lanes
// stride the tile, a butterfly over the wave, waves in order, tiles in order, planes in a fixed tree).  No atomics.
//
// Work split: one workgroup per (plane, 16 x 16 tile of pixels).  A pixel's gradient needs the up-to-49 windows that contain it (top-left
// corners 6 up and left of it) and those need the pixels 6 further down and right: the workgroup stages a 28 x 28 window of x and y (fp32,
// widened when read: the same doubles), forms the 22 x 28 vertical sums of x, y, x^2, y^2, xy, then S and the three gradient maps
// (alpha, beta, gamma) of its 22 x 22 windows -- zero for a window outside the interior --, then the vertical and horizontal 7-sums of the
// maps.  The windows whose corner lies in the tile are the ones it owns for the loss.  LDS: 2 x 28 x 28 x 4 (x, y) + 5 x 22 x 28 x 8 (vertical
// sums, reused for the maps' vertical sums) + 3 x 22 x 22 x 8 (maps) + 32 = 42,560 bytes: three workgroups (12 waves) per CU of 160 KiB.
// With grad == nullptr only the owned windows are evaluated and the second pass is skipped.

#include "loss_common.hip.inc"

namespace ssimloss {

constexpr int TH = 16, TW = 16;            // pixels (and owned window corners) per tile
constexpr int PH = TH + 12, PW = TW + 12;  // staged pixels: 6 before the tile (the windows that reach into it), 6 behind (their extent)
constexpr int WH = TH + 6, WW = TW + 6;    // windows per tile, by top-left corner, starting 6 before the tile
constexpr int THREADS = 256;

constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, COV_NORM = 49.0 / 48.0, TWO_COV_NORM = 2.0 * (49.0 / 48.0);

using losscommon::wave_sum;

__global__ __launch_bounds__(THREADS)
void tile_loss_grad(const float* __restrict__ pred, const float* __restrict__ gt, double* __restrict__ part, float* __restrict__ grad,
                    int H, int W, int nby, int nbx, double divisor) {
#pragma clang fp contract(off)
    __shared__ float sx[PH * PW], sy[PH * PW];        // x = pred', y = gt'; 0 outside the plane (never read by a window inside the interior)
    __shared__ double sv[5][WH * PW];                 // vertical 7-row sums of x, y, x^2, y^2, xy; later [3][TH * WW]: those of the maps
    __shared__ double sm[3][WH * WW];                 // alpha, beta, gamma per window
    __shared__ double red[THREADS / 64];
    const int tile = blockIdx.x;
    const int bx = tile % nbx, by = (tile / nbx) % nby;
    const long long plane = tile / (nbx * nby);
    const int r0 = by * TH, c0 = bx * TW, Ho = H - 6, Wo = W - 6;
    const float* p = pred + plane * H * W;
    const float* g = gt + plane * H * W;

    for (int i = threadIdx.x; i < PH * PW; i += THREADS) {
        const int lr = i / PW, lc = i - lr * PW, r = r0 - 6 + lr, c = c0 - 6 + lc;
        float xv = 0.f, yv = 0.f;
        if (r >= 0 && r < H && c >= 0 && c < W) {
            xv = (p[(long long)r * W + c] + 1.f) / 2.f;
            yv = (g[(long long)r * W + c] + 1.f) / 2.f;
        }
        sx[i] = xv;
        sy[i] = yv;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < WH * PW; i += THREADS) {
        const int wr = i / PW, lc = i - wr * PW;
        double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const double x = (double)sx[(wr + k) * PW + lc], y = (double)sy[(wr + k) * PW + lc];
            a = a + x; b = b + y; aa = aa + x * x; bb = bb + y * y; ab = ab + x * y;
        }
        sv[0][i] = a; sv[1][i] = b; sv[2][i] = aa; sv[3][i] = bb; sv[4][i] = ab;
    }
    __syncthreads();
    double ssim = 0.0;
    for (int i = threadIdx.x; i < WH * WW; i += THREADS) {
        const int wr = i / WW, wc = i - wr * WW, wi = r0 - 6 + wr, wj = c0 - 6 + wc;
        const bool owned = wr >= 6 && wc >= 6;
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        if (wi >= 0 && wi < Ho && wj >= 0 && wj < Wo && (owned || grad != nullptr)) {
            double s[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < 7; ++k) t = t + sv[q][wr * PW + wc + k];
                s[q] = t;
            }
            const double ux = s[0] / 49.0, uy = s[1] / 49.0, uxx = s[2] / 49.0, uyy = s[3] / 49.0, uxy = s[4] / 49.0;
            const double vx = COV_NORM * (uxx - ux * ux), vy = COV_NORM * (uyy - uy * uy), vxy = COV_NORM * (uxy - ux * uy);
            const double A1 = (2.0 * ux) * uy + C1, A2 = 2.0 * vxy + C2;
            const double B1 = (ux * ux + uy * uy) + C1, B2 = (vx + vy) + C2;
            const double D = B1 * B2;
            const double S = (A1 * A2) / D;
            if (owned) ssim += S;
            gamma = -((TWO_COV_NORM * S) / B2);
            beta = (TWO_COV_NORM * A1) / D;
            alpha = ((((2.0 * uy) * A2) / D - ((2.0 * S) * ux) / B1) - beta * uy) - gamma * ux;
        }
        sm[0][i] = alpha; sm[1][i] = beta; sm[2][i] = gamma;
    }
    ssim = wave_sum(ssim);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ssim;
    __syncthreads();          // (also: every read of sv above is done, every map is written)
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < THREADS / 64; ++w) t += red[w];
        part[tile] = t;
    }
    if (grad == nullptr) return;

    double (*sa)[TH * WW] = reinterpret_cast<double (*)[TH * WW]>(&sv[0][0]);
    for (int i = threadIdx.x; i < TH * WW; i += THREADS) {
        const int pr = i / WW, wc = i - pr * WW;      // pixel row r0 + pr: the windows of rows r0 + pr - 6 + k, k = 0..6
        double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            a = a + sm[0][(pr + k) * WW + wc]; b = b + sm[1][(pr + k) * WW + wc]; c = c + sm[2][(pr + k) * WW + wc];
        }
        sa[0][i] = a; sa[1][i] = b; sa[2][i] = c;
    }
    __syncthreads();
    float* gp = grad + plane * H * W;
    for (int i = threadIdx.x; i < TH * TW; i += THREADS) {
        const int pr = i / TW, pc = i - pr * TW, r = r0 + pr, c = c0 + pc;
        if (r >= H || c >= W) continue;
        double a = 0.0, b = 0.0, cc = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            a = a + sa[0][pr * WW + pc + k]; b = b + sa[1][pr * WW + pc + k]; cc = cc + sa[2][pr * WW + pc + k];
        }
        const double x = (double)sx[(pr + 6) * PW + pc + 6], y = (double)sy[(pr + 6) * PW + pc + 6];
        const double d = ((a + y * b) + x * cc) / 49.0;
        gp[(long long)r * W + c] = (float)((-0.5 * d) / divisor);
    }
}

// One thread per plane: its tiles in order, then the interior mean.
__global__ __launch_bounds__(THREADS)
void finish_planes(const double* __restrict__ part, double* __restrict__ plane_ssim, int planes, int tiles, int H, int W) {
#pragma clang fp contract(off)
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= planes) return;
    const double interior = (double)(H - 6) * (double)(W - 6);
    const double* q = part + (long long)n * tiles;
    double s = 0.0;
    for (int t = 0; t < tiles; ++t) s += q[t];
    plane_ssim[n] = s / interior;
}

// One workgroup: lane t sums the planes t, t + 256, ... in order, then a fixed halving tree; a function of the plane count alone.
__global__ __launch_bounds__(THREADS)
void finish_total(const double* __restrict__ plane_ssim, double* __restrict__ totals, int planes) {
#pragma clang fp contract(off)
    __shared__ double acc[THREADS];
    double s = 0.0;
    for (int n = threadIdx.x; n < planes; n += THREADS) s += plane_ssim[n];
    acc[threadIdx.x] = s;
    __syncthreads();
    for (int h = THREADS / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) acc[threadIdx.x] = acc[threadIdx.x] + acc[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mean = acc[0] / (double)planes;
        totals[0] = mean;
        totals[1] = 1.0 - mean;
    }
}

struct Plan {
    int nby, nbx;
    long long tiles_total;    // N * C * nby * nbx
};

inline Plan plan(int N, int C, int H, int W) {
    Plan p;
    p.nby = (H + TH - 1) / TH;
    p.nbx = (W + TW - 1) / TW;
    p.tiles_total = (long long)N * C * p.nby * p.nbx;
    return p;
}

// what tai_ssim_loss and its workspace query refuse for the dimensions; null: they are taken.  (The launcher's alignment message sits
// between the size checks and the tile count, where it always has; the query has no pointers and passes nothing.)
inline const char* refusal(int N, int C, int H, int W, bool pointers_aligned = true) {
    if (N <= 0 || C <= 0 || H < 7 || W < 7) return "ssim_loss: needs N, C >= 1 and H, W >= 7 (the 7x7 SSIM window)";
    if ((long long)N * C * H * W >= (1LL << 40) || (long long)H * W >= (1LL << 31)) return "ssim_loss: tensor too large";
    if (!pointers_aligned) return "ssim_loss: workspace, plane_ssim and totals must be 8-byte aligned";
    if (plan(N, C, H, W).tiles_total >= (1LL << 31)) return "ssim_loss: too many tiles (2^31 or more)";
    return nullptr;
}

}  // namespace ssimloss
