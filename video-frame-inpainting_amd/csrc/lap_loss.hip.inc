// Laplacian-pyramid L1 loss and its gradient in one launch (included by sepconv_capi.hip); the definition is the one
// include/tai_sepconv.h writes down for tai_lap_loss and tests/lap_loss_ref.py restates in numpy:
//   d = (pred + 1) / 2 - (gt + 1) / 2 in fp32 (util.inverse_transform), NOT clipped, then float64 for everything below;
//   G_0 = d, G_{l+1} = D(G_l): taps (1, 4, 6, 4, 1) / 16 at stride 2, edges replicated, rows then columns, each 5-term sum left to right;
//   L_l = G_l - U(G_{l+1}) below the top, L_{L-1} = G_{L-1}: U's taps (1, 6, 1) / 8 at even and (4, 4) / 8 at odd indices;
//   loss = sum_l 2^l sum |L_l| / (P H W);  grad = fp32(t_0 * 0.5 / (P H W)), t_0 the adjoint pyramid of the signs 2^l sign(L_l).
//
// Exactness: a Laplacian value is a fixed-order float64 expression of its plane's pixels with contraction off.  Every value of the
// adjoint pyramid is a dyadic rational that float64 holds exactly for L <= 6, so its sums have no order to keep and the gradient is
// rounded once: a pixel's gradient bits depend on its plane and on (P, H, W, L) only.  Only the order of the sums of |L_l| belongs to
// the kernel (a lane's pixels in order, a butterfly over the wave, waves in order); the totals add the planes in plane order.  No atomics.
//
// Work split: the levels depend on each other and a plane's coarse levels are tiny, so ONE workgroup of 1024 lanes owns a plane and
// walks the levels with workgroup barriers; the grid is capped at GRID_CAP workgroups, past it a workgroup strides over the planes.
// G_0 is never stored: it is recomputed from pred and gt where it is needed.  Levels 1..L-1 share one float64 array of about a third
// of a plane that holds, in turn and in place, G_l, then s_l = 2^l sign(L_l), then t_l: a level's Laplacian reads G_l at its own pixel
// only, and the adjoint at level l reads s_{l-1} and t_{l+1} and writes level l, going down.  The level-0 signs are parked in grad as
// floats (-1, 0, 1 are exact) and replaced by the gradient in the last pass.  The array lives in LDS when it fits (62 KB: a 128 x 128
// plane needs 43.5 KB), otherwise in the caller's workspace, one slice per workgroup, which stays in L2.  D and U are evaluated on
// the fly per output pixel (25 and up to 9 reads), their adjoints as gathers over the 25 and 9 candidate pixels with the operators'
// weights, which takes care of every clamped edge, 1 x 1 levels included.

#include "loss_common.hip.inc"

namespace laploss {

constexpr int THREADS = 1024;
constexpr int MAXL = 6;
constexpr int LDS_DOUBLES = 7936;          // 62 KB: two workgroups per CU
constexpr int GRID_CAP = 512;              // two workgroups on each of 256 CUs
constexpr int FIN_THREADS = 256;

constexpr double K0 = 1.0 / 16.0, K1 = 4.0 / 16.0, K2 = 6.0 / 16.0;

struct Args {
    const float* pred;
    const float* gt;
    float* grad;                           // may be null: evaluation only
    double* plane_terms;                   // [planes][levels]
    double* work;                          // [grid][pyramid] when the pyramid does not fit LDS
    long long planes;
    double count;                          // P H W
    int levels;
    int pyramid;                           // doubles of levels 1..L-1
    int h[MAXL], w[MAXL], off[MAXL];       // level sizes; where level l >= 1 starts in the pyramid array
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

using losscommon::wave_sum;

// every lane gets the workgroup's sum: the waves in order
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) t += red[k];
    __syncthreads();
    return t;
}

// sign(0) = +0, a NaN kept
__device__ __forceinline__ double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v)); }

// G_0 at (r, c): the fp32 difference of the range-mapped frames, widened
struct Diff {
    const float* p;
    const float* g;
    int w;
    __device__ __forceinline__ double operator()(int r, int c) const {
#pragma clang fp contract(off)
        const long long i = (long long)r * w + c;
        const float x = (p[i] + 1.f) / 2.f, y = (g[i] + 1.f) / 2.f;
        return (double)(x - y);
    }
};

template <class T>
struct Level {
    const T* q;
    int w;
    __device__ __forceinline__ double operator()(int r, int c) const { return (double)q[r * w + c]; }
};

// D at (i, j) of the next level, from a level of h x w
template <class Src>
__device__ __forceinline__ double reduce_at(const Src& src, int i, int j, int h, int w) {
#pragma clang fp contract(off)
    const int r0 = clampi(2 * i - 2, h - 1), r1 = clampi(2 * i - 1, h - 1), r2 = 2 * i, r3 = clampi(2 * i + 1, h - 1),
              r4 = clampi(2 * i + 2, h - 1);
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        const int c = clampi(2 * j + b - 2, w - 1);
        double t = K0 * src(r0, c);
        t = t + K1 * src(r1, c);
        t = t + K2 * src(r2, c);
        t = t + K1 * src(r3, c);
        t = t + K0 * src(r4, c);
        const double k = b == 0 || b == 4 ? K0 : (b == 2 ? K2 : K1);
        acc = b == 0 ? k * t : acc + k * t;
    }
    return acc;
}

// U's row pass at fine row r, coarse column j, from a level of mh rows
template <class Src>
__device__ __forceinline__ double expand_rows(const Src& src, int r, int j, int mh) {
#pragma clang fp contract(off)
    const int i = r >> 1, after = clampi(i + 1, mh - 1);
    if (r & 1) return src(i, j) / 2.0 + src(after, j) / 2.0;
    return (src(clampi(i - 1, mh - 1), j) / 8.0 + (6.0 * src(i, j)) / 8.0) + src(after, j) / 8.0;
}

// U at (r, c) of the level below, from a level of mh x mw
template <class Src>
__device__ __forceinline__ double expand_at(const Src& src, int r, int c, int mh, int mw) {
#pragma clang fp contract(off)
    const int j = c >> 1, after = clampi(j + 1, mw - 1);
    if (c & 1) return expand_rows(src, r, j, mh) / 2.0 + expand_rows(src, r, after, mh) / 2.0;
    return (expand_rows(src, r, clampi(j - 1, mw - 1), mh) / 8.0 + (6.0 * expand_rows(src, r, j, mh)) / 8.0) +
           expand_rows(src, r, after, mh) / 8.0;
}

// the weight of coarse index i in U's output f (m coarse entries); exact
__device__ __forceinline__ double up_weight(int f, int i, int m) {
    const int h = f >> 1, after = clampi(h + 1, m - 1);
    if (f & 1) return (h == i ? 0.5 : 0.0) + (after == i ? 0.5 : 0.0);
    return ((clampi(h - 1, m - 1) == i ? 0.125 : 0.0) + (h == i ? 0.75 : 0.0)) + (after == i ? 0.125 : 0.0);
}

// the weight of fine index f in D's output i (n fine entries); exact
__device__ __forceinline__ double down_weight(int i, int f, int n) {
    double w = 0.0;
#pragma unroll
    for (int a = 0; a < 5; ++a)
        if (clampi(2 * i + a - 2, n - 1) == f) w += a == 0 || a == 4 ? K0 : (a == 2 ? K2 : K1);
    return w;
}

// U^T(s)(i, j): s on the fine level fh x fw, (i, j) on the coarse level mh x mw; exact sums.  The outputs of U that read coarse index i
// are 2i - 2 .. 2i + 2; the weights of the rows and of the columns are formed once.
template <class Src>
__device__ __forceinline__ double expand_adjoint_at(const Src& s, int i, int j, int fh, int fw, int mh, int mw) {
    double wr[5], wc[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int fr = 2 * i - 2 + k, fc = 2 * j - 2 + k;
        wr[k] = fr >= 0 && fr < fh ? up_weight(fr, i, mh) : 0.0;
        wc[k] = fc >= 0 && fc < fw ? up_weight(fc, j, mw) : 0.0;
    }
    double u = 0.0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        if (wr[a] == 0.0) continue;
        double row = 0.0;
#pragma unroll
        for (int b = 0; b < 5; ++b)
            if (wc[b] != 0.0) row += wc[b] * s(2 * i - 2 + a, 2 * j - 2 + b);
        u += wr[a] * row;
    }
    return u;
}

// D^T(t)(r, c): t on the coarse level mh x mw, (r, c) on the fine level fh x fw; exact sums.  The outputs of D that read fine index r
// are r/2 - 1 .. r/2 + 1 (the clamped reads of the first and the last output included).
template <class Src>
__device__ __forceinline__ double reduce_adjoint_at(const Src& t, int r, int c, int fh, int fw, int mh, int mw) {
    const int i0 = (r >> 1) - 1, j0 = (c >> 1) - 1;
    double wr[3], wc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        wr[k] = i0 + k >= 0 && i0 + k < mh ? down_weight(i0 + k, r, fh) : 0.0;
        wc[k] = j0 + k >= 0 && j0 + k < mw ? down_weight(j0 + k, c, fw) : 0.0;
    }
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (wr[a] == 0.0) continue;
        double row = 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (wc[b] != 0.0) row += wc[b] * t(i0 + a, j0 + b);
        v += wr[a] * row;
    }
    return v;
}

// One plane, by the whole workgroup.  buf: the pyramid array (LDS or a workspace slice); ends with a barrier, so buf can be reused.
__device__ __forceinline__ void plane_pyramid(const Args& a, double* buf, double* red, long long plane) {
#pragma clang fp contract(off)
    const int L = a.levels, H = a.h[0], W = a.w[0], tid = threadIdx.x;
    const long long base = plane * H * W;
    const Diff d0{a.pred + base, a.gt + base, W};
    float* gr = a.grad ? a.grad + base : nullptr;

    // the Gaussian pyramid
    for (int l = 1; l < L; ++l) {
        const int h = a.h[l], w = a.w[l], n = h * w, ph = a.h[l - 1], pw = a.w[l - 1];
        double* out = buf + a.off[l];
        const Level<double> below{buf + a.off[l - 1], pw};
        for (int idx = tid; idx < n; idx += THREADS) {
            const int i = idx / w, j = idx - i * w;
            out[idx] = l == 1 ? reduce_at(d0, i, j, ph, pw) : reduce_at(below, i, j, ph, pw);
        }
        __syncthreads();
    }

    // the Laplacians going up: sums of |L_l|, the signs in place of G_l
    for (int l = 0; l < L; ++l) {
        const int h = a.h[l], w = a.w[l], n = h * w;
        double* own = buf + a.off[l];                  // (unused at l == 0)
        const Level<double> above{buf + (l + 1 < L ? a.off[l + 1] : 0), l + 1 < L ? a.w[l + 1] : 0};
        const double scale = (double)(1 << l);
        double sum = 0.0;
        for (int idx = tid; idx < n; idx += THREADS) {
            const int r = idx / w, c = idx - r * w;
            double v = l == 0 ? d0(r, c) : own[idx];
            if (l + 1 < L) v = v - expand_at(above, r, c, a.h[l + 1], a.w[l + 1]);
            sum += fabs(v);
            if (gr) {
                if (l == 0) gr[idx] = (float)sgn(v);
                else own[idx] = scale * sgn(v);
            }
        }
        // (the barriers inside: nobody reads level l + 1 through U any more when the next pass overwrites it)
        const double total = block_sum(sum, red);
        if (tid == 0) a.plane_terms[plane * L + l] = total;
    }
    if (!gr) return;

    // the adjoint pyramid going down: level l becomes t_l = (s_l - U^T(s_{l-1})) + D^T(t_{l+1})
    for (int l = L - 1; l >= 1; --l) {
        const int h = a.h[l], w = a.w[l], n = h * w, fh = a.h[l - 1], fw = a.w[l - 1];
        double* own = buf + a.off[l];
        const Level<float> signs0{gr, fw};
        const Level<double> signs{buf + a.off[l - 1], fw};
        const Level<double> above{buf + (l + 1 < L ? a.off[l + 1] : 0), l + 1 < L ? a.w[l + 1] : 0};
        for (int idx = tid; idx < n; idx += THREADS) {
            const int i = idx / w, j = idx - i * w;
            const double u = l == 1 ? expand_adjoint_at(signs0, i, j, fh, fw, h, w) : expand_adjoint_at(signs, i, j, fh, fw, h, w);
            double v = own[idx] - u;
            if (l + 1 < L) v = v + reduce_adjoint_at(above, i, j, h, w, a.h[l + 1], a.w[l + 1]);
            own[idx] = v;
        }
        __syncthreads();
    }
    {
        const Level<double> above{buf + (L > 1 ? a.off[1] : 0), L > 1 ? a.w[1] : 0};
        const int n = H * W;
        for (int idx = tid; idx < n; idx += THREADS) {
            const int r = idx / W, c = idx - r * W;
            double v = (double)gr[idx];
            if (L > 1) v = v + reduce_adjoint_at(above, r, c, H, W, a.h[1], a.w[1]);
            gr[idx] = (float)((v * 0.5) / a.count);
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(THREADS)
void pyramid_lds(const Args a) {
    __shared__ double buf[LDS_DOUBLES];
    __shared__ double red[THREADS / 64];
    for (long long plane = blockIdx.x; plane < a.planes; plane += gridDim.x) plane_pyramid(a, buf, red, plane);
}

__global__ __launch_bounds__(THREADS)
void pyramid_workspace(const Args a) {
    __shared__ double red[THREADS / 64];
    double* buf = a.work + (long long)blockIdx.x * a.pyramid;
    for (long long plane = blockIdx.x; plane < a.planes; plane += gridDim.x) plane_pyramid(a, buf, red, plane);
}

// One workgroup: the planes in plane order (staged through LDS 256 planes at a time, lane l adds level l's), then the terms and the loss.
__global__ __launch_bounds__(FIN_THREADS)
void finish_total(const double* __restrict__ plane_terms, double* __restrict__ totals, long long planes, int levels, double count) {
#pragma clang fp contract(off)
    __shared__ double chunk[FIN_THREADS * MAXL];
    __shared__ double term[MAXL];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long first = 0; first < planes; first += FIN_THREADS) {
        const int rows = (int)(planes - first < FIN_THREADS ? planes - first : FIN_THREADS);
        for (int k = tid; k < rows * levels; k += FIN_THREADS) chunk[k] = plane_terms[first * levels + k];
        __syncthreads();
        if (tid < levels)
            for (int q = 0; q < rows; ++q) s += chunk[q * levels + tid];
        __syncthreads();
    }
    if (tid < levels) {
        term[tid] = ((double)(1 << tid) * s) / count;
        totals[tid] = term[tid];
    }
    __syncthreads();
    if (tid == 0) {
        double loss = term[0];
        for (int l = 1; l < levels; ++l) loss = loss + term[l];
        totals[levels] = loss;
    }
}

// what tai_lap_loss and its workspace query refuse for the dimensions; null: they are taken
inline const char* refusal(long long planes, int H, int W, int levels) {
    if (planes < 1) return "lap_loss: needs at least one plane";
    if (levels < 1 || levels > MAXL) return "lap_loss: levels must be 1..6 (past 6 the gradient's adjoint sums are no longer exact in float64)";
    if (H < 1 || W < 1 || (H < W ? H : W) < (1 << (levels - 1))) return "lap_loss: needs min(H, W) >= 2^(levels-1)";
    const long long hw = (long long)H * W;
    if (hw >= (1LL << 31) || planes > ((1LL << 31) - 1) / hw) return "lap_loss: tensor too large (planes H W >= 2^31)";
    return nullptr;
}

struct Plan {
    Args a;                   // the sizes filled in
    bool in_lds;
    unsigned grid;
    long long work_bytes;     // never 0, so that a caller can always allocate it
};

inline Plan plan(long long planes, int H, int W, int levels) {
    Plan p{};
    p.a.planes = planes;
    p.a.levels = levels;
    p.a.count = ((double)planes * (double)H) * (double)W;
    int off = 0;
    for (int l = 0; l < levels; ++l) {
        p.a.h[l] = l == 0 ? H : (p.a.h[l - 1] + 1) / 2;
        p.a.w[l] = l == 0 ? W : (p.a.w[l - 1] + 1) / 2;
        p.a.off[l] = off;
        if (l >= 1) off += p.a.h[l] * p.a.w[l];
    }
    p.a.pyramid = off;
    p.in_lds = off <= LDS_DOUBLES;
    p.grid = (unsigned)(planes < GRID_CAP ? planes : GRID_CAP);
    p.work_bytes = p.in_lds ? 8 : (long long)p.grid * off * (long long)sizeof(double);
    return p;
}

}  // namespace laploss
