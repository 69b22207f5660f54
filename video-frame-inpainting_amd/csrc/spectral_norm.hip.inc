// Spectral-norm power iteration and in-place renormalisation of one discriminator layer (included by sepconv_capi.hip).
//
// The reference's SNConv2d / SNLinear (src/discriminators/SNDiscriminator.py:10-25, 60-68, 84-92) run, on EVERY forward,
// Ip rounds of  v <- normalise(u W),  u <- normalise(v W^T),  then sigma = (v W^T) u^T  and  W.data <- W.data / sigma.
// One training step at K=T=F=5 evaluates the discriminator on 13 windows x 3 passes x 5 layers = 195 such calls; as ATen
// ops that is ~30 tiny kernels per call (a third of all launches of the step, and the [1,512] x [512,4096] products go
// to a GEMM library tile that takes 90 us each).  Here a call is 2 Ip + 1 launches:
//   wt_u   : v_raw[j] = sum_o W[o][j] u[o]          (/ (|u| + eps) when u is an unnormalised product)
//   w_v    : t_raw[o] = sum_j W[o][j] v_raw[j] / (|v_raw| + eps)
//   finish : u <- t_raw / (|t_raw| + eps), sigma = sum_o t_raw[o] u[o], W <- W / sigma
// The normalisation of a vector is applied by its consumer (the products are linear in it), so no kernel waits on a
// grid-wide norm.  All sums have a fixed order: the results are reproducible from call to call.

#include "loss_common.hip.inc"

namespace snorm {

constexpr float EPS = 1e-12f;      // _l2normalize's eps (SNDiscriminator.py:27-28)

using losscommon::wave_sum;

// Sum over the whole workgroup (blockDim.x * blockDim.y threads, a multiple of 64, at most 1024); every thread gets it.
__device__ __forceinline__ float block_sum(float x, float* red) {
    const int t = threadIdx.y * blockDim.x + threadIdx.x, nw = (blockDim.x * blockDim.y) >> 6;
    x = wave_sum(x);
    __syncthreads();                       // red may still be read from a previous call
    if ((t & 63) == 0) red[t >> 6] = x;
    __syncthreads();
    float s = 0.f;
    for (int w = 0; w < nw; ++w) s += red[w];
    return s;
}

constexpr int WT_COLS = 64, WT_ROWGROUPS = 16;

// v_raw[j] = scale * sum_o W[o][j] u[o]; scale = 1 / (|u| + eps) if normalise.  Block (64, 16): 64 columns, rows dealt
// round-robin to 16 row groups, partial sums combined through LDS in a fixed order.
__global__ __launch_bounds__(WT_COLS * WT_ROWGROUPS)
void wt_u(const float* __restrict__ W, const float* __restrict__ u, float* __restrict__ v_raw, int out_rows, int in_cols,
          int normalise) {
    __shared__ float red[16];
    __shared__ float part[WT_ROWGROUPS][WT_COLS];
    float scale = 1.f;
    if (normalise) {
        float ss = 0.f;
        for (int o = threadIdx.y * WT_COLS + threadIdx.x; o < out_rows; o += WT_COLS * WT_ROWGROUPS) ss += u[o] * u[o];
        scale = 1.f / (sqrtf(block_sum(ss, red)) + EPS);
    }
    const int col = blockIdx.x * WT_COLS + threadIdx.x;
    float acc = 0.f;
    if (col < in_cols)
        for (int o = threadIdx.y; o < out_rows; o += WT_ROWGROUPS) acc += W[(long long)o * in_cols + col] * u[o];
    part[threadIdx.y][threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.y == 0 && col < in_cols) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < WT_ROWGROUPS; ++g) s += part[g][threadIdx.x];
        v_raw[col] = s * scale;
    }
}

// t_raw[o] = sum_j W[o][j] v_raw[j] / (|v_raw| + eps): one workgroup of 256 per row.
__global__ __launch_bounds__(256)
void w_v(const float* __restrict__ W, const float* __restrict__ v_raw, float* __restrict__ t_raw, int in_cols) {
    __shared__ float red[16];
    const float* row = W + (long long)blockIdx.x * in_cols;
    float dot = 0.f, ss = 0.f;
    if (in_cols % 4 == 0) {
        for (int j = threadIdx.x; j < in_cols / 4; j += 256) {
            const float4 w = reinterpret_cast<const float4*>(row)[j], v = reinterpret_cast<const float4*>(v_raw)[j];
            dot += w.x * v.x + w.y * v.y + w.z * v.z + w.w * v.w;
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
    } else {
        for (int j = threadIdx.x; j < in_cols; j += 256) { dot += row[j] * v_raw[j]; ss += v_raw[j] * v_raw[j]; }
    }
    dot = block_sum(dot, red);
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) t_raw[blockIdx.x] = dot / (sqrtf(ss) + EPS);
}

// u <- t_raw / (|t_raw| + eps); sigma = sum_o t_raw[o] u[o]; W <- W / sigma (every workgroup derives sigma itself).
__global__ __launch_bounds__(256)
void finish(float* __restrict__ W, const float* __restrict__ t_raw, float* __restrict__ u, float* __restrict__ sigma_out,
            int out_rows, long long n) {
    __shared__ float red[16];
    float ss = 0.f;
    for (int o = threadIdx.x; o < out_rows; o += 256) ss += t_raw[o] * t_raw[o];
    const float inv = 1.f / (sqrtf(block_sum(ss, red)) + EPS);
    float dot = 0.f;
    for (int o = threadIdx.x; o < out_rows; o += 256) dot += t_raw[o] * (t_raw[o] * inv);
    const float sigma = block_sum(dot, red);
    if (blockIdx.x == 0) {
        for (int o = threadIdx.x; o < out_rows; o += 256) u[o] = t_raw[o] * inv;
        if (threadIdx.x == 0 && sigma_out) *sigma_out = sigma;
    }
    const long long stride = (long long)gridDim.x * 256;
    if (n % 4 == 0) {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += stride) {
            float4 w = reinterpret_cast<float4*>(W)[i];
            w.x /= sigma; w.y /= sigma; w.z /= sigma; w.w /= sigma;
            reinterpret_cast<float4*>(W)[i] = w;
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) W[i] /= sigma;
    }
}

// The element-wise tail of a discriminator layer evaluated on all windows at once (sn_discriminator._WindowScaledConv): the
// convolution ran with the weight w0 of before the windows' renormalisations, window t's weight is w0 * inv_scale[t], so
//   y = leaky_relu(conv * inv_scale[window] + bias[channel], slope)                          (in place, one pass)
// and backwards, from the gradient g of that output and the output itself,
//   gz = g * (y > 0 ? 1 : slope)     -- the gradient of the layer's pre-activation: weight and bias gradients take it as it is
//   gs = gz * inv_scale[window]      -- what flows on into the input gradient (through w0)
// ATen ran these as three and two passes over [13 B, C, H, W].  x: [nw * B, C, HW] contiguous, HW % 4 == 0 (any HW: the _scalar forms).
__global__ __launch_bounds__(256)
void window_scale_bias_lrelu(float* __restrict__ y, const float* __restrict__ bias, const float* __restrict__ inv_scale,
                             long long n4, int chw4, int hw4, int C, int B, float slope) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const int w = (int)(i / ((long long)chw4 * B));
        const float s = inv_scale[w], b = bias[(int)((i / hw4) % C)];
        float4 v = reinterpret_cast<float4*>(y)[i];
        v.x = v.x * s + b; v.y = v.y * s + b; v.z = v.z * s + b; v.w = v.w * s + b;
        v.x = v.x > 0.f ? v.x : v.x * slope; v.y = v.y > 0.f ? v.y : v.y * slope;
        v.z = v.z > 0.f ? v.z : v.z * slope; v.w = v.w > 0.f ? v.w : v.w * slope;
        reinterpret_cast<float4*>(y)[i] = v;
    }
}

__global__ __launch_bounds__(256)
void window_scale_lrelu_backward(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ inv_scale,
                                 float* __restrict__ gz, float* __restrict__ gs, long long n4, int chw4, int B, float slope) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float s = inv_scale[(int)(i / ((long long)chw4 * B))];
        const float4 a = reinterpret_cast<const float4*>(g)[i], o = reinterpret_cast<const float4*>(y)[i];
        float4 z;
        z.x = o.x > 0.f ? a.x : a.x * slope; z.y = o.y > 0.f ? a.y : a.y * slope;
        z.z = o.z > 0.f ? a.z : a.z * slope; z.w = o.w > 0.f ? a.w : a.w * slope;
        reinterpret_cast<float4*>(gz)[i] = z;
        reinterpret_cast<float4*>(gs)[i] = make_float4(z.x * s, z.y * s, z.z * s, z.w * s);
    }
}

// The same two passes one element per thread, for planes with HW % 4 != 0 (the 10 x 13 output of the last layer at 160 x 208
// frames), where a 4-element group would straddle two channels.  A workgroup walks whole planes (plane = (window, image, channel)):
// the window's factor and the channel's bias are found once per plane, the pixels of a plane are 32-bit offsets.  The arithmetic
// per element is the one above.
__global__ __launch_bounds__(256)
void window_scale_bias_lrelu_scalar(float* __restrict__ y, const float* __restrict__ bias, const float* __restrict__ inv_scale,
                                    int planes, int hw, int C, int B, float slope) {
    for (int p = blockIdx.x; p < planes; p += gridDim.x) {
        const float s = inv_scale[p / (C * B)], b = bias[p % C];
        float* yp = y + (long long)p * hw;
        for (int i = threadIdx.x; i < hw; i += 256) {
            const float v = yp[i] * s + b;
            yp[i] = v > 0.f ? v : v * slope;
        }
    }
}

__global__ __launch_bounds__(256)
void window_scale_lrelu_backward_scalar(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ inv_scale,
                                        float* __restrict__ gz, float* __restrict__ gs, int planes, int hw, int C, int B, float slope) {
    for (int p = blockIdx.x; p < planes; p += gridDim.x) {
        const float s = inv_scale[p / (C * B)];
        const long long o = (long long)p * hw;
        for (int i = threadIdx.x; i < hw; i += 256) {
            const float z = y[o + i] > 0.f ? g[o + i] : g[o + i] * slope;
            gz[o + i] = z;
            gs[o + i] = z * s;
        }
    }
}

}  // namespace snorm
