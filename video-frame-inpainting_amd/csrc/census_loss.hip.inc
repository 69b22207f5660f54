// Census (soft ternary) loss and its gradient for up to three predictions against one ground truth, in one launch (included by
// sepconv_capi.hip); the definition is the one include/tai_sepconv.h writes down for tai_census_loss and tests/census_loss_ref.py restates
// in numpy:
//   I = gray((pred + 1) / 2), J = gray((gt + 1) / 2) in fp32, NOT clipped; for the 48 offsets j of the 7 x 7 window, in row-major order:
//   s = 255 * (I(q+j) - I(q)), u = 0.81 + s * s, r = sqrt(u), t = s / r (s', t' from J);  d = t - t', e = d * d, n = 0.1 + e, phi = e / n;
//   dphi = ((2 * d) * 0.1) / (n * n), tau = 0.81 / (u * r), w = (double)dphi * (double)tau;
//   D(q) = (sum_j (double)phi) / 49 for q in the interior Omega (3 pixels off every edge);  frame term = the mean of D over Omega;
//   G(q) = -sum_j m(q, j) * w(q, j), m = [q in Omega] + [q+j in Omega], over the j with q + j in the plane;  grad = fp32(G * kappa).
//
// Exactness: a pixel's gradient is a fixed expression of the pixel's own 7 x 7 neighbourhood and kappa, with contraction off (the term
// window q - k sends to q is w(q-k, k) = -w(q, -k) bit for bit, so there is no scatter and no second pass): it does not depend on the
// tiling, the other frames, npred, the other predictions or the strides.  Only the order of the float64 sum of D over a frame belongs to
// the kernel (a lane's four pixels left to right, a butterfly over the wave, waves in order, tiles in order).  No atomics.
//
// Work split: one workgroup per (frame, 32 x 32 tile of the plane), 256 lanes, a lane owns four consecutive pixels of one row and takes them
// one after the other.  The workgroup stages the intensity of the tile and its 3-pixel halo, cut to the plane, once for the ground truth and
// once per prediction: 38 rows of ten 4-pixel runs from column c0 - 4 on (a run starts at a multiple of four columns: one 16-byte load per
// channel where the run is whole and its address a multiple of 16, single words otherwise), the gray conversion on the way.  LDS row
// stride 41 words: the four rows a half-wave reads start at banks 0, 41, 18, 59, apart modulo 4, so its 32 lanes (bank 4 * lane + const
// within a row) never meet.  The ground truth's (s', t') of an offset is computed once and used by every prediction.  One 16-byte store
// per gradient channel where the run allows.  LDS: 4 x 38 x 41 x 4 + 96 = 25,024 bytes (25,040 with the float64 slots' alignment): six
// workgroups per CU.  The kernel is bound by the vector ALU (per pixel, offset and prediction a square root and four divisions, all
// correctly rounded, plus the ground truth's share), not by bandwidth.  The grid is capped at GRID_CAP workgroups; past it a workgroup
// strides over the tiles.

#include "loss_common.hip.inc"

namespace censusloss {

constexpr int TH = 32, TW = 32;            // pixels per tile (of the plane, not of the interior)
constexpr int THREADS = 256;               // TH rows x (TW / 4) lanes
constexpr int R = 3;                       // the window reaches R pixels each way
constexpr int SH = TH + 2 * R;             // staged rows: r0 - 3 .. r0 + TH + 2
constexpr int RUNS = (TW + 8) / 4;         // staged 4-pixel runs per row: columns c0 - 4 .. c0 + TW + 3
constexpr int LW = 41;                     // LDS row stride in words (>= 4 * RUNS; see above)
constexpr int MAXP = 3;
constexpr long long GRID_CAP = 1LL << 14;

struct Args {
    const float* pred[MAXP];
    float* grad[MAXP];                     // any may be null
    const float* gt;
    long long sb[MAXP + 1], st[MAXP + 1];  // batch and time stride in elements; the ground truth's at [MAXP]
    double* part;                          // [npred][frames * tiles per frame]
    int npred, T, C, H, W, nby, nbx;
    long long tiles_total;                 // frames * nby * nbx
    double kappa;                          // (255 * 0.5) / (49 * count)
};

using namespace losscommon;

// util.gray01's weights, in its operand order
constexpr float GRAY0 = 0.1140f, GRAY1 = 0.5870f, GRAY2 = 0.2989f;

// the first nv (0..4) words of the run at q; the others read as zero
__device__ __forceinline__ void load_run(const float* q, int nv, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (nv == 4 && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        // volatile: the compiler may not move a word's load out of (or below) both branches, which would turn the 16-byte load above
        // into a 4-byte and a 12-byte one
        const volatile float* w = q;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) v[j] = w[j];
    }
}

__device__ __forceinline__ void store_run(float* q, int nv, const float (&g)[4]) {
    if (nv == 4 && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
        *reinterpret_cast<float4*>(q) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
        volatile float* w = q;          // (as in load_run)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) w[j] = g[j];
    }
}

// One frame's intensity over the tile and its halo into s[SH][LW]: item = staged row * RUNS + run.  Words outside the plane are not
// written and never read.
template <int C>
__device__ __forceinline__ void stage(const float* __restrict__ frame, float* __restrict__ s, int r0, int c0, int H, int W) {
#pragma clang fp contract(off)
    const long long plane = (long long)H * W;
    for (int item = threadIdx.x; item < SH * RUNS; item += THREADS) {
        const int lr = item / RUNS, run = item - lr * RUNS;
        const int r = r0 - R + lr, c = c0 - 4 + 4 * run;
        if (r < 0 || r >= H || c < 0 || c >= W) continue;
        const int nv = W - c < 4 ? W - c : 4;
        const float* q = frame + (long long)r * W + c;
        float v[4];
        load_run(q, nv, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = range_map(v[j]);
        if (C == 3) {
            float v1[4], v2[4];
            load_run(q + plane, nv, v1);
            load_run(q + 2 * plane, nv, v2);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (GRAY0 * v[j] + GRAY1 * range_map(v1[j])) + GRAY2 * range_map(v2[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) s[lr * LW + 4 * run + j] = v[j];
    }
}

// s = 255 (a - b), u = 0.81 + s s, r = sqrt(u), t = s / r
__device__ __forceinline__ void soft_sign(float a, float b, float& u, float& r, float& t) {
#pragma clang fp contract(off)
    const float s = 255.f * (a - b);
    u = 0.81f + s * s;
    r = __builtin_sqrtf(u);
    t = s / r;
}

template <int C>
__global__ __launch_bounds__(THREADS)
void tile_loss_grad(const Args a) {
#pragma clang fp contract(off)
    __shared__ float sj[SH * LW];
    __shared__ float si[MAXP][SH * LW];
    __shared__ double red[MAXP][THREADS / 64];
    const int H = a.H, W = a.W, npred = a.npred;
    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
    const int wave = threadIdx.x >> 6;
    const long long plane = (long long)H * W;
    // tiles, frames and a frame's tiles all stay below 2^31 (refusal()): 32-bit divisions
    const unsigned tiles_total = (unsigned)a.tiles_total, tiles_per_frame = (unsigned)(a.nby * a.nbx);

    for (unsigned tile = blockIdx.x; tile < tiles_total; tile += gridDim.x) {
        const unsigned f = tile / tiles_per_frame, within = tile - f * tiles_per_frame;
        const int by = (int)(within / (unsigned)a.nbx), bx = (int)(within - (unsigned)by * (unsigned)a.nbx);
        const unsigned bu = f / (unsigned)a.T;
        const long long b = bu, t = f - bu * (unsigned)a.T;
        const int r0 = by * TH, c0 = bx * TW;

        stage<C>(a.gt + b * a.sb[MAXP] + t * a.st[MAXP], sj, r0, c0, H, W);
#pragma unroll
        for (int i = 0; i < MAXP; ++i)
            if (i < npred) stage<C>(a.pred[i] + b * a.sb[i] + t * a.st[i], si[i], r0, c0, H, W);
        __syncthreads();

        const int r = r0 + ty, c = c0 + 4 * tx;
        const int nv = (r < H && c < W) ? (W - c < 4 ? W - c : 4) : 0;          // pixels of the lane's run inside the plane
        const bool row_in = r >= R && r < H - R;
        double frame_sum[MAXP] = {0.0, 0.0, 0.0};
        float g[MAXP][C][4];
#pragma unroll
        for (int i = 0; i < MAXP; ++i)
#pragma unroll
            for (int k = 0; k < C; ++k) g[i][k][0] = g[i][k][1] = g[i][k][2] = g[i][k][3] = 0.f;

        for (int p = 0; p < nv; ++p) {
            const int x = c + p;
            const bool q_in = row_in && x >= R && x < W - R;
            const int centre = (ty + R) * LW + 4 + 4 * tx + p;
            const float jq = sj[centre];
            float iq[MAXP];
            double phi_sum[MAXP] = {0.0, 0.0, 0.0}, acc[MAXP] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int i = 0; i < MAXP; ++i) iq[i] = i < npred ? si[i][centre] : 0.f;
            for (int dy = -R; dy <= R; ++dy) {
                const int yy = r + dy;
                if (yy < 0 || yy >= H) continue;
                const bool yy_in = yy >= R && yy < H - R;
#pragma unroll
                for (int dx = -R; dx <= R; ++dx) {
                    const int xx = x + dx;
                    if ((dx == 0 && dy == 0) || xx < 0 || xx >= W) continue;
                    const double m = (double)((int)q_in + (int)(yy_in && xx >= R && xx < W - R));
                    const int at = centre + dy * LW + dx;
                    float up, rp, tp;
                    soft_sign(sj[at], jq, up, rp, tp);
#pragma unroll
                    for (int i = 0; i < MAXP; ++i) {
                        if (i >= npred) continue;
                        float u, rr, tt;
                        soft_sign(si[i][at], iq[i], u, rr, tt);
                        const float d = tt - tp;
                        const float e = d * d;
                        const float n = 0.1f + e;
                        const float phi = e / n;
                        const float dphi = ((2.f * d) * 0.1f) / (n * n);
                        const float tau = 0.81f / (u * rr);
                        const double w = (double)dphi * (double)tau;
                        phi_sum[i] = phi_sum[i] + (double)phi;
                        acc[i] = acc[i] + m * w;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < MAXP; ++i) {
                if (q_in) frame_sum[i] = frame_sum[i] + phi_sum[i] / 49.0;          // off Omega the window is not whole and no D exists
                const double gk = (-acc[i]) * a.kappa;
                const float wk[3] = {GRAY0, GRAY1, GRAY2};
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const float v = C == 1 ? (float)gk : (float)(gk * (double)wk[k]);          // rounded once
                    g[i][k][0] = p == 0 ? v : g[i][k][0];
                    g[i][k][1] = p == 1 ? v : g[i][k][1];
                    g[i][k][2] = p == 2 ? v : g[i][k][2];
                    g[i][k][3] = p == 3 ? v : g[i][k][3];
                }
            }
        }

#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            if (i >= npred) continue;
            if (a.grad[i] != nullptr && nv > 0) {
                float* q = a.grad[i] + b * a.sb[i] + t * a.st[i] + (long long)r * W + c;
#pragma unroll
                for (int k = 0; k < C; ++k) store_run(q + k * plane, nv, g[i][k]);
            }
            const double s = wave_sum(frame_sum[i]);
            if ((threadIdx.x & 63) == 0) red[i][wave] = s;
        }
        __syncthreads();
        if ((int)threadIdx.x < npred) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < THREADS / 64; ++w) s = s + red[threadIdx.x][w];
            a.part[(long long)threadIdx.x * a.tiles_total + tile] = s;
        }
        // the next tile's staging starts behind this barrier (every lane's window reads are done), and its `red` writes behind the next
        // one, which these lanes reach after their reads: nothing is overwritten early
    }
}

// One thread per (prediction, frame): the frame's tiles in order, divided by the number of interior pixels.
__global__ __launch_bounds__(THREADS)
void finish_frames(const double* __restrict__ part, double* __restrict__ frame_terms, long long rows, int tiles_per_frame, double interior) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;        // i * frames + f
    if (n >= rows) return;
    const double* q = part + n * tiles_per_frame;                                // tile index i * tiles_total + f * tiles_per_frame
    double acc = 0.0;
    for (int k = 0; k < tiles_per_frame; ++k) acc = acc + q[k];
    frame_terms[n] = acc / interior;
}

// One workgroup per prediction: the frame terms in frame order.  256 at a time go through LDS (one coalesced load), and lane 0 adds them
// one after the other: the sum is the sequential one, whatever the frame count.
__global__ __launch_bounds__(THREADS)
void finish_total(const double* __restrict__ frame_terms, double* __restrict__ totals, long long frames) {
#pragma clang fp contract(off)
    __shared__ double chunk[THREADS];
    const double* q = frame_terms + (long long)blockIdx.x * frames;
    double acc = 0.0;
    for (long long f0 = 0; f0 < frames; f0 += THREADS) {
        const long long left = frames - f0;
        const int n = left < THREADS ? (int)left : THREADS;
        if ((int)threadIdx.x < n) chunk[threadIdx.x] = q[f0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < n; ++k) acc = acc + chunk[k];
        __syncthreads();          // chunk is read before the next 256 are written
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = acc / (double)frames;
}

struct Plan {
    int nby, nbx;
    long long frames, tiles_total;
};

inline Plan plan(int B, int T, int H, int W) {
    Plan p;
    p.nby = (H + TH - 1) / TH;
    p.nbx = (W + TW - 1) / TW;
    p.frames = (long long)B * T;
    p.tiles_total = p.frames * p.nby * p.nbx;
    return p;
}

// what tai_census_loss and its workspace query refuse for the dimensions; null: they are taken
inline const char* refusal(int npred, int B, int T, int C, int H, int W) {
    if (npred < 1 || npred > MAXP) return "census_loss: npred must be 1, 2 or 3";
    if (B < 1 || T < 1 || C < 1 || H < 1 || W < 1) return "census_loss: needs B, T, C, H, W >= 1";
    if (C != 1 && C != 3) return "census_loss: C must be 1 (gray) or 3";
    if (H < 2 * R + 1 || W < 2 * R + 1) return "census_loss: needs H, W >= 7 (the 7x7 window)";
    const long long hw = (long long)H * W, frames = (long long)B * T;
    if (hw >= (1LL << 31) || C * hw > ((1LL << 40) - 1) / frames)
        return "census_loss: tensor too large (B T C H W >= 2^40 or H W >= 2^31)";
    if (frames >= (1LL << 31) || plan(B, T, H, W).tiles_total >= (1LL << 31)) return "census_loss: too many frames or tiles (2^31 or more)";
    return nullptr;
}

// everything tai_census_loss refuses, before any runtime call; null: the launch goes ahead
inline const char* call_refusal(const float* const* preds, int npred, const float* gt, const long long* strides, const double* frame_terms,
                                const double* totals, const void* workspace, int B, int T, int C, int H, int W) {
    if (!preds || !gt || !strides || !frame_terms || !totals || !workspace) return "census_loss: null pointer";
    if (const char* why = refusal(npred, B, T, C, H, W)) return why;
    for (int i = 0; i < npred; ++i)
        if (!preds[i]) return "census_loss: null prediction pointer";
    const long long chw = (long long)C * H * W;
    for (int i = 0; i <= npred; ++i)
        switch (block_strides_fault(strides[2 * i], strides[2 * i + 1], B, T, chw)) {
            case STRIDES_NOT_POSITIVE: return "census_loss: strides must be positive";
            case STRIDES_REACH_2_40: return "census_loss: strides reach an offset of 2^40 elements or more";
            case STRIDES_OVERLAP: return "census_loss: strides under which two (b, t) blocks overlap";
        }
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(frame_terms) % 8 || reinterpret_cast<uintptr_t>(totals) % 8)
        return "census_loss: workspace, frame_terms and totals must be 8-byte aligned";
    return nullptr;
}

}  // namespace censusloss
