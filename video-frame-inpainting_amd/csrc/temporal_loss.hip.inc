// Temporal-difference loss (L2 / L1 / Charbonnier of the frame-to-frame difference of the error, the known frames on both sides of the
// gap included) and its gradient for up to three predictions against one ground truth, in one launch (included by sepconv_capi.hip); the
// definition is the one include/tai_sepconv.h writes down for tai_temporal_loss and tests/temporal_loss_ref.py restates in numpy:
//   x = (pred + 1) / 2, y = (gt + 1) / 2, e_t = x_t - y_t in fp32 (util.inverse_transform), NOT clipped; e_{-1} = e_T = +0;
//   d_j = e_j - e_{j-1} for j = 0..T;  rho(d) = d * d | |d| | sqrt(d * d + eps * eps);  rho'(d) = 2 * d | sgn(d) | d / sqrt(d * d + eps * eps);
//   sums of rho(d_j) per sequence (b, c) and position j in float64;  grad_t = fp32(((double)rho'(d_t) - (double)rho'(d_{t+1})) * ct).
//
// Exactness: a pixel's gradient is a fixed expression of the pixel's own T values and ct, with contraction off: it does not depend on the
// split into chunks, the other sequences, npred, the other predictions or the strides.  Only the order of the float64 sums belongs to the
// kernel (a lane's four pixels left to right, a butterfly over the wave, then waves, chunks and sequences in a fixed order).  No atomics.
//
// Work split: a sequence's H x ceil(W / 4) runs of four consecutive pixels of a row are cut into chunks of 256; one workgroup per chunk,
// one run per lane.  The lane walks t = 0..T with e_{t-1} and rho'(d_{t-1}) of its four pixels in registers: frame t + 1 is loaded before
// frame t's arithmetic, every input element is read once (gt once for all predictions) and frame t - 1 of every gradient is written once,
// at step t.  16-byte loads and stores where the run is whole and its address is a multiple of 16 (checked per tensor and frame: the
// strides decide), single words otherwise.  Addresses are b * sb + t * st + c * H * W + r * W + col with the tensor's own (sb, st).  No LDS
// and no barrier: each wave's sum of position j goes to the workspace, [npred][chunks][T + 1][4].  The grid is capped at GRID_CAP
// workgroups; past it a workgroup strides over the chunks.

#include "loss_common.hip.inc"

namespace temploss {

constexpr int THREADS = 256;               // runs per chunk
constexpr int WAVES = THREADS / 64;
constexpr int MAXP = 3;
constexpr long long GRID_CAP = 1LL << 20;

struct Args {
    const float* pred[MAXP];
    float* grad[MAXP];                     // any may be null
    const float* gt;
    long long sb[MAXP + 1], st[MAXP + 1];  // batch and time stride in elements; the ground truth's at [MAXP]
    double* part;                          // [npred][chunks_total][T + 1][WAVES]
    int npred, kind, T, C, H, W;
    int rpr, cps;                          // runs per row, chunks per sequence
    long long runs;                        // H * rpr, per sequence
    long long chunks_total;                // S * cps
    float e2;                              // eps * eps in fp32
    double ct;                             // 0.5 / count
};

using namespace losscommon;

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

__global__ __launch_bounds__(THREADS)
void walk_loss_grad(const Args a) {
#pragma clang fp contract(off)
    const int T = a.T, W = a.W, npred = a.npred;
    const long long plane = (long long)a.H * W;
    const int wave = threadIdx.x >> 6;
    const bool writer = (threadIdx.x & 63) == 0;

    // chunks, sequences and a sequence's runs (rounded up to whole chunks) all stay below 2^32 (refusal()): 32-bit divisions
    const unsigned chunks_total = (unsigned)a.chunks_total, runs = (unsigned)a.runs;
    for (unsigned chunk = blockIdx.x; chunk < chunks_total; chunk += gridDim.x) {
        const unsigned s = chunk / (unsigned)a.cps;
        const unsigned n = (chunk - s * (unsigned)a.cps) * THREADS + threadIdx.x;          // the lane's run of its sequence
        const bool live = n < runs;
        const int r = live ? (int)(n / (unsigned)a.rpr) : 0;
        const int c0 = live ? 4 * (int)(n - (unsigned)r * (unsigned)a.rpr) : 0;
        const int nv = live ? (W - c0 < 4 ? W - c0 : 4) : 0;                      // pixels of the run inside the row; 0: the lane only sums
        const unsigned bu = s / (unsigned)a.C;
        const long long b = bu, c = s - bu * (unsigned)a.C;
        const long long in_block = c * plane + (long long)r * W + c0;
        const float* gq = a.gt + b * a.sb[MAXP] + in_block;
        const float* pq[MAXP];
        float* dq[MAXP];
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            pq[i] = i < npred ? a.pred[i] + b * a.sb[i] + in_block : nullptr;
            dq[i] = (i < npred && a.grad[i] != nullptr) ? a.grad[i] + b * a.sb[i] + in_block : nullptr;
        }

        float yc[4], xc[MAXP][4], yn[4], xn[MAXP][4];
        float e_prev[MAXP][4], dr_prev[MAXP][4];
        load_run(gq, nv, yc);
        yn[0] = yn[1] = yn[2] = yn[3] = 0.f;
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { xc[i][j] = 0.f; xn[i][j] = 0.f; e_prev[i][j] = 0.f; dr_prev[i][j] = 0.f; }
            if (i < npred) load_run(pq[i], nv, xc[i]);
        }

        for (int t = 0; t <= T; ++t) {
            if (t + 1 < T) {                                                      // the next frame, before this one's arithmetic
                load_run(gq + (long long)(t + 1) * a.st[MAXP], nv, yn);
#pragma unroll
                for (int i = 0; i < MAXP; ++i)
                    if (i < npred) load_run(pq[i] + (long long)(t + 1) * a.st[i], nv, xn[i]);
            }
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = range_map(yc[j]);
#pragma unroll
            for (int i = 0; i < MAXP; ++i) {
                if (i >= npred) continue;
                double sum = 0.0;
                float g[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float e = t < T ? range_map(xc[i][j]) - y[j] : 0.f;     // e_T = +0: the known frame after the gap
                    const float d = e - e_prev[i][j];                             // d_t; e_{-1} = +0
                    float rho, drho;
                    rho_drho(a.kind, d, a.e2, rho, drho);
                    if (j < nv) sum = sum + (double)rho;
                    g[j] = (float)(((double)dr_prev[i][j] - (double)drho) * a.ct);          // frame t - 1's
                    e_prev[i][j] = e;
                    dr_prev[i][j] = drho;
                }
                if (t > 0 && dq[i] != nullptr && nv > 0) store_run(dq[i] + (long long)(t - 1) * a.st[i], nv, g);
                sum = wave_sum(sum);
                if (writer) a.part[(((long long)i * a.chunks_total + (long long)chunk) * (T + 1) + t) * WAVES + wave] = sum;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                yc[j] = yn[j];
#pragma unroll
                for (int i = 0; i < MAXP; ++i) xc[i][j] = xn[i][j];
            }
        }
    }
}

// One thread per (prediction, sequence, position): the sequence's chunks in order, the four waves of each in order.
__global__ __launch_bounds__(THREADS)
void finish_sequences(const double* __restrict__ part, double* __restrict__ seq_terms, long long rows, long long S, int T1, int cps) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;        // (i * S + s) * T1 + j
    if (n >= rows) return;
    const long long is = n / T1;
    const int j = (int)(n - is * T1);
    const double* q = part + (is * cps * T1 + j) * WAVES;                         // chunk index i * chunks_total + s * cps = (i * S + s) * cps
    double acc = 0.0;
    for (int k = 0; k < cps; ++k) {
#pragma unroll
        for (int w = 0; w < WAVES; ++w) acc += q[w];
        q += (long long)T1 * WAVES;
    }
    seq_terms[n] = acc;
}

// One workgroup per prediction, position after position: lane t sums the sequences t, t + 256, ... in order, then a fixed halving tree; a
// function of the sequence count alone.  The loss is the sum of the positions' sums in order, divided once.
__global__ __launch_bounds__(THREADS)
void finish_total(const double* __restrict__ seq_terms, double* __restrict__ totals, long long S, int T1, double n_pos, double count) {
#pragma clang fp contract(off)
    __shared__ double acc[THREADS];
    const double* q = seq_terms + (long long)blockIdx.x * S * T1;
    double* out = totals + (long long)blockIdx.x * (T1 + 1);
    double all = 0.0;
    for (int j = 0; j < T1; ++j) {
        double p = 0.0;
        for (long long s = threadIdx.x; s < S; s += THREADS) p += q[s * T1 + j];
        acc[threadIdx.x] = p;
        __syncthreads();
        for (int h = THREADS / 2; h >= 1; h >>= 1) {
            if ((int)threadIdx.x < h) acc[threadIdx.x] = acc[threadIdx.x] + acc[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            out[j] = acc[0] / n_pos;
            all = all + acc[0];
        }
        __syncthreads();          // acc[0] is read before position j + 1 writes it
    }
    if (threadIdx.x == 0) out[T1] = all / count;
}

struct Plan {
    int rpr, cps;
    long long runs, chunks_total;
};

inline Plan plan(long long S, int H, int W) {
    Plan p;
    p.rpr = (W + 3) / 4;
    p.runs = (long long)H * p.rpr;
    p.cps = (int)((p.runs + THREADS - 1) / THREADS);
    p.chunks_total = S * p.cps;
    return p;
}

// what tai_temporal_loss and its workspace query refuse for the dimensions; null: they are taken
inline const char* refusal(int npred, int B, int T, int C, int H, int W) {
    if (npred < 1 || npred > MAXP) return "temporal_loss: npred must be 1, 2 or 3";
    if (B < 1 || T < 1 || C < 1 || H < 1 || W < 1) return "temporal_loss: needs B, T, C, H, W >= 1";
    const long long hw = (long long)H * W, S = (long long)B * C;
    if (hw >= (1LL << 31) || S > ((1LL << 40) - 1) / hw || S * hw > ((1LL << 40) - 1) / T)
        return "temporal_loss: tensor too large (B T C H W >= 2^40 or H W >= 2^31)";
    if (S * ((long long)T + 1) >= (1LL << 31)) return "temporal_loss: too many sequence positions (B C (T + 1) >= 2^31)";
    if (plan(S, H, W).chunks_total >= (1LL << 31)) return "temporal_loss: too many chunks (2^31 or more)";
    return nullptr;
}

// One tensor's strides (losscommon::block_strides_fault), in this entry's words.
inline const char* stride_refusal(long long sb, long long st, int B, int T, long long chw) {
    switch (block_strides_fault(sb, st, B, T, chw)) {
        case STRIDES_NOT_POSITIVE: return "temporal_loss: strides must be positive";
        case STRIDES_REACH_2_40: return "temporal_loss: strides reach an offset of 2^40 elements or more";
        case STRIDES_OVERLAP: return "temporal_loss: strides under which two (b, t) blocks overlap";
    }
    return nullptr;
}

// everything tai_temporal_loss refuses, before any runtime call; null: the launch goes ahead
inline const char* call_refusal(const float* const* preds, int npred, const float* gt, const long long* strides, int kind, float eps,
                                const double* seq_terms, const double* totals, const void* workspace, int B, int T, int C, int H, int W) {
    if (!preds || !gt || !strides || !seq_terms || !totals || !workspace) return "temporal_loss: null pointer";
    if (const char* why = refusal(npred, B, T, C, H, W)) return why;
    if (kind < 0 || kind > 2) return "temporal_loss: kind must be 0 (L2), 1 (L1) or 2 (Charbonnier)";
    if (kind == 2 && !(std::isfinite(eps) && eps > 0.f)) return "temporal_loss: the Charbonnier eps must be finite and > 0";
    for (int i = 0; i < npred; ++i)
        if (!preds[i]) return "temporal_loss: null prediction pointer";
    const long long chw = (long long)C * H * W;
    for (int i = 0; i <= npred; ++i)
        if (const char* why = stride_refusal(strides[2 * i], strides[2 * i + 1], B, T, chw)) return why;
    if (reinterpret_cast<uintptr_t>(workspace) % 8 || reinterpret_cast<uintptr_t>(seq_terms) % 8 || reinterpret_cast<uintptr_t>(totals) % 8)
        return "temporal_loss: workspace, seq_terms and totals must be 8-byte aligned";
    return nullptr;
}

}  // namespace temploss
