/*
 * tai_sepconv.h -- C ABI of the MI355X-native adaptive separable convolution.
 *
 * Drop-in boundary for the reference's only native component.  Each entry point
 * replaces one symbol of the reference's cffi-exported C shim:
 *
 *   tai_sepconv_forward   <- int SeparableConvolution_cuda_forward(THCudaTensor* input, vertical,
 *                            horizontal, output, int ks)
 *                            src/separable_convolution/cfile/SeparableConvolution_cuda.h:1-7
 *                            (body cuda.c:8-25 -> launcher SeparableConvolution_kernel.cu:164-185)
 *   tai_sepconv_backward  <- int SeparableConvolution_cuda_backward(grad_output, input, vertical,
 *                            horizontal, grad_input, grad_vertical, grad_horizontal, int ks)
 *                            src/separable_convolution/cfile/SeparableConvolution_cuda.h:9-18
 *                            (body cuda.c:28-51 -> launcher SeparableConvolution_kernel.cu:187-242)
 *
 * THC tensor handles no longer exist (torch >= 1.0), so tensors cross the boundary as raw device
 * pointers plus their dimensions.  Conventions kept from the reference:
 *   - the CALLER owns and pre-allocates every buffer, outputs included; the callee only writes
 *     (SeparableConvolution.py:36,69-71).  Outputs need not be zeroed: every element is written.
 *   - all tensors are contiguous fp32 NCHW on the device the stream belongs to;
 *   - the call is asynchronous on `stream` (the reference used the THC current stream) and does
 *     no host synchronisation, allocation or copy, so it can be captured into a hipGraph.
 * Convention changed: the reference returned 1 unconditionally and reported launch failures through
 * THCudaCheck; these functions return TAI_SEPCONV_OK (0) or a negative TAI_SEPCONV_E* code, and
 * tai_sepconv_last_error() gives the text.
 *
 * Shapes (Hp = H + ks - 1, Wp = W + ks - 1; the reference asserts exactly this relation,
 * SeparableConvolution.py:27-29):
 *   input       [B, C, Hp, Wp]   replication-padded source frame
 *   vertical    [B, ks, H, W]    per-pixel vertical taps
 *   horizontal  [B, ks, H, W]    per-pixel horizontal taps
 *   output      [B, C, H, W]     out[b,c,y,x] = sum_fy sum_fx in[b,c,y+fy,x+fx] v[b,fy,y,x] h[b,fx,y,x]
 *   grad_*      same shapes as the tensor they are the gradient of.
 */
#ifndef TAI_SEPCONV_H
#define TAI_SEPCONV_H

#ifdef __cplusplus
extern "C" {
#endif

#define TAI_SEPCONV_OK 0
#define TAI_SEPCONV_EINVAL (-1)  /* null pointer, non-positive dimension, index space >= 2^31 */
#define TAI_SEPCONV_ELAUNCH (-2) /* hipGetLastError() after a launch was not hipSuccess */

/* Forward: replaces SeparableConvolution_cuda_forward (SeparableConvolution_cuda.h:1-7). */
int tai_sepconv_forward(const float* input, const float* vertical, const float* horizontal,
                        float* output, int B, int C, int H, int W, int ks, void* hip_stream);

/* Backward (all three gradients, in the reference's V, H, I order):
 * replaces SeparableConvolution_cuda_backward (SeparableConvolution_cuda.h:9-18).
 * Any of grad_input / grad_vertical / grad_horizontal may be NULL to skip that gradient.
 * Precondition: every operand is finite.  The grad_input strips kernel lets window positions outside a source row hold
 * other rows' values and cancels them by multiplying with a zero tap (csrc/sepconv_bwd.hip.inc: they hold finite values
 * and meet S = 0); an Inf or NaN there would reach gradients it does not belong to. */
int tai_sepconv_backward(const float* grad_output, const float* input, const float* vertical,
                         const float* horizontal, float* grad_input, float* grad_vertical,
                         float* grad_horizontal, int B, int C, int H, int W, int ks,
                         void* hip_stream);

/* Bilinear x2 upsampling, align_corners = true, fp32 NCHW with planes = N*C: output [planes, 2H, 2W].
 * Replaces the THCUNN kernel behind the reference's torch.nn.Upsample(scale_factor=2, mode='bilinear') calls
 * (src/models/tai/tai.py:283,337,343; torch 0.3.1 semantics = align_corners=True), same caller-allocates / asynchronous-
 * on-stream conventions as above. */
int tai_upsample_bilinear2x_forward(const float* input, float* output, int planes, int H, int W, void* hip_stream);
/* Its gradient: grad_output [planes, 2H, 2W] -> grad_input [planes, H, W] (every element written), as a gather with the
 * forward's weights; sums in a fixed order (ATen's backward scatters with atomics). */
int tai_upsample_bilinear2x_backward(const float* grad_output, float* grad_input, int planes, int H, int W, void* hip_stream);

/* In-place x[n,c,:] = act(x[n,c,:] + bias[c]) over a contiguous fp32 [N, C, HW] tensor; act: 0 none, 1 ReLU, 2 tanh.
 * Finishes the bias-free MIOpen convolutions of the generator in one pass (the reference's nn.Conv2d + nn.ReLU / nn.Tanh
 * pairs, src/models/mcnet/mcnet.py:28-43,79-102,137-144,172-176,203-225; src/models/tai/tai.py:256-261). */
int tai_bias_act_inplace(float* x, const float* bias, int N, int C, int HW, int act, void* hip_stream);

/* out [planes, 2h, 2w] = res + fixed_unpooling(x), x [planes, h, w] landing on the even (2i, 2j) sites (DecCnn:
 * src/models/mcnet/mcnet.py:234-236, 240-256); fp32 contiguous, w even; out may not alias x or res. */
int tai_unpool2x_add(const float* x, const float* res, float* out, long long planes, int h, int w, void* hip_stream);

/* ConvLSTM gate arithmetic in one pass (ConvLstmCell.forward, src/models/mcnet/mcnet.py:287-293): gates [N, 4F, HW] holds the
 * chunks (i, j, f, o) of conv(cat(input, h)); c, new_c, new_h are [N, F, HW]; HW % 4 == 0.
 *   new_c = c * sigmoid(f + forget_bias) + sigmoid(i) * tanh(j);   new_h = tanh(new_c) * sigmoid(o). */
int tai_convlstm_gates_forward(const float* gates, const float* c, float* new_c, float* new_h, int N, int F, int HW,
                               float forget_bias, void* hip_stream);
/* Its gradient: from dL/dnew_c and dL/dnew_h (either may be NULL: no gradient on that path) to grad_gates [N, 4F, HW] and
 * grad_c [N, F, HW]; gates, c and new_c as in the forward call. */
int tai_convlstm_gates_backward(const float* gates, const float* c, const float* new_c, const float* grad_new_c,
                                const float* grad_new_h, float* grad_gates, float* grad_c, int N, int F, int HW, float forget_bias,
                                void* hip_stream);

/* Direct "same"-padded stride-1 convolutions for the generator's thin layers, bias and activation fused (act: 0 none,
 * 1 ReLU, 2 tanh), fp32 NCHW contiguous, W % 4 == 0:
 *   tai_conv_cin1_forward       x [N,1,H,W], weight [Co,1,k,k] (k in {3,5}), y [N,Co,H,W]   (nn.Conv2d(1, gf, 5, padding=2)
 *                               + ReLU, src/models/mcnet/mcnet.py:28-31; nn.Conv2d(c_dim=1, gf, 3, padding=1) + ReLU, :79-81)
 *   tai_conv_cout1_3x3_forward  x [N,Ci,H,W], weight [1,Ci,3,3] in conv2d layout, y [N,1,H,W]
 *                               (nn.ConvTranspose2d(gf, c_dim=1, 3, padding=1) + Tanh, mcnet.py:223-224, after the
 *                               transpose-and-flip that turns it into a direct convolution). */
int tai_conv_cin1_forward(const float* x, const float* weight, const float* bias, float* y, int N, int Co, int H, int W,
                          int k, int act, void* hip_stream);
/* tai_conv_cin1_forward that also writes ypool [N,Co,H/2,W/2] = 2x2 max pool of the activated output (even H). */
int tai_conv_cin1_forward_maxpool(const float* x, const float* weight, const float* bias, float* y, float* ypool, int N, int Co,
                                  int H, int W, int k, int act, void* hip_stream);
/* ... with ypool written into a plane of pool_h x pool_w whose origin is at (pool_oy, pool_ox):
 * the halo-carrying input plane of the next layer (tai_conv3x3_wino_forward_ex, shift_k), halo left untouched. */
int tai_conv_cin1_forward_maxpool_window(const float* x, const float* weight, const float* bias, float* y, float* ypool, int N,
                                         int Co, int H, int W, int k, int act, int pool_h, int pool_w, int pool_oy, int pool_ox,
                                         void* hip_stream);
int tai_conv_cout1_3x3_forward(const float* x, const float* weight, const float* bias, float* y, int N, int Ci, int H,
                               int W, int act, void* hip_stream);
/* ... 5 x 5, padding 2, no activation, bias may be NULL: x [N,Ci,H,W], weight [1,Ci,5,5] -> y [N,1,H,W]; the input gradient of
 * tai_conv_cin1_forward (k = 5) when the input frame is itself generated (weight = the layer's filter flipped). */
int tai_conv_cout1_5x5_forward(const float* x, const float* weight, const float* bias, float* y, int N, int Ci, int H, int W,
                               void* hip_stream);

/* k x k (k = 5, 7) "same" convolution as a 3x3 convolution: out [N, S*S*C, H+2, W+4] (S = 2 for k = 5, 3 for k = 7)
 * receives the S*S shifted copies of x [N, C, H, W], each with its own halo -- out[n][(a*S+b)*C+c][u][v] =
 * x[n][c][u-1+3a-k/2+1][v-2+3b-k/2+1], zero outside the image -- and the k x k weight, cut into S x S blocks of 3 x 3 taps
 * ([K, S*S*C, 3, 3], zero past k), is then an ordinary weight for tai_conv3x3_wino_transform_weights; the convolution is
 * tai_conv3x3_wino_forward_window(out, ..., in_h = H+2, in_w = W+4, in_oy = 1, in_ox = 2).  Replaces
 * nn.Conv2d(gf, 2gf, 5, padding=2) and nn.Conv2d(2gf, 4gf, 7, padding=3) of MotionEnc (src/models/mcnet/mcnet.py:36-38,
 * 45-47).  W % 4 == 0. */
int tai_conv_shift_stack(const float* x, float* out, int N, int C, int H, int W, int k, void* hip_stream);

/* Element-wise tail of a discriminator layer evaluated on all sliding windows at once (nw window groups of B images stacked
 * along the batch; window t's weight is w0 * inv_scale[t], src/discriminators/SNDiscriminator.py:60-68, 140-159):
 *   forward, in place:  y = leaky_relu(y * inv_scale[window] + bias[channel], slope)          y [nw * B, C, HW], HW % 4 == 0
 *   backward:  grad_z = grad_y * (y > 0 ? 1 : slope)  (the pre-activation's gradient: weight / bias gradients take it),
 *              grad_scaled = grad_z * inv_scale[window]  (what flows into the input gradient through w0). */
int tai_window_scale_bias_lrelu(float* y, const float* bias, const float* inv_scale, int nw, int B, int C, int HW, float slope,
                                void* hip_stream);
/* The same two passes for any HW >= 1, one element per thread (the 10 x 13 output of the last layer at 160 x 208 frames). */
int tai_window_scale_bias_lrelu_scalar(float* y, const float* bias, const float* inv_scale, int nw, int B, int C, int HW, float slope,
                                       void* hip_stream);
int tai_window_scale_lrelu_backward_scalar(const float* grad_y, const float* y, const float* inv_scale, float* grad_z, float* grad_scaled,
                                           int nw, int B, int C, int HW, float slope, void* hip_stream);
int tai_window_scale_lrelu_backward(const float* grad_y, const float* y, const float* inv_scale, float* grad_z, float* grad_scaled,
                                    int nw, int B, int C, int HW, float slope, void* hip_stream);

/* Weight and bias gradients of the thin layers (tai_conv_cin1_forward / tai_conv_cout1_3x3_forward under loss.backward()):
 *   dw[cb][a][b] = sum over n, y, x of big[n, cb, y, x] * thin[n, 0, y + a - k/2, x + b - k/2]  (zero padding),  dbias[cb] = sum of big[n, cb]
 * big [N, Cb, H, W], thin [N, 1, H, W] fp32 contiguous, W % 4 == 0, k in {3, 5}; dw [Cb, k, k] or dbias [Cb] may be NULL;
 * workspace: N * Cb * 32 floats.  One-input-channel convolution: big = dL/dy, thin = x.  One-output-channel convolution:
 * big = x, thin = dL/dy, and dw[c][a][b] is the gradient of weight[0][c][k-1-a][k-1-b].  Reproducible (fixed summation order). */
int tai_thin_conv_wrw(const float* big, const float* thin, float* dw, float* dbias, float* workspace, int N, int Cb, int H, int W,
                      int k, void* hip_stream);

/* Activation + 2x2 max pool behind a convolution, training form (nn.ReLU + nn.MaxPool2d(2) of ContentEnc / MotionEnc,
 * src/models/mcnet/mcnet.py:28-60, 79-118): z, y [planes, H, W], ypool [planes, H/2, W/2] fp32 contiguous, H even, W % 4 == 0.
 *   forward:  y = relu ? max(z, 0) : z;  ypool = max over each 2x2 window of y                     (y may alias z)
 *   backward: grad_z = (relu ? [y > 0] : 1) * (grad_y + grad_ypool routed to the first maximum of its window in row-major
 *             order, nn.MaxPool2d's tie rule); grad_y or grad_ypool may be NULL (that path carries no gradient). */
int tai_act_maxpool2x2_forward(const float* z, float* y, float* ypool, long long planes, int H, int W, int relu, void* hip_stream);
int tai_act_maxpool2x2_backward(const float* grad_y, const float* grad_ypool, const float* y, float* grad_z, long long planes, int H,
                                int W, int relu, void* hip_stream);

/* Weight gradient of the 3x3 stride-1 padding-1 convolution y = conv(x, w) (the reference's nn.Conv2d / ConvTranspose2d
 * 3x3 layers under loss.backward(), src/environments/environments.py:348-355), in the Winograd domain on the fp32 MFMA pipe:
 *   dw [K, C, 3, 3] = sum over n, y, x of dy[n, k, y, x] * x[n, c, y + a - 1, x + b - 1]      (zero padding)
 * and, when dbias is not NULL, the bias gradient dbias [K] = sum over n, y, x of dy[n, k, y, x] (the output gradient
 * passes through the kernel anyway).
 * x [N, C, H, W], dy [N, K, H, W] fp32 contiguous, any H, W >= 1, each tensor below 2 GiB.  Shapes other than even H with
 * W % 16 == 0 are computed on both planes zero-extended to an even number of rows and roundup(W, 16) columns (inside the
 * kernel, no copy; exact: the added output-gradient pixels are zeros).  workspace: device memory
 * of tai_conv3x3_wino_wrw_workspace_floats(...) floats (-1: shape not supported), overwritten.  Partial sums of the
 * workgroups are combined in a fixed order: the results are reproducible from call to call. */
long long tai_conv3x3_wino_wrw_workspace_floats(int N, int C, int K, int H, int W);
int tai_conv3x3_wino_wrw(const float* x, const float* dy, float* dw, float* dbias, float* workspace, int N, int C, int K, int H,
                         int W, void* hip_stream);
/* ... with x given as a plane of in_h x in_w per channel whose pixel (in_oy, in_ox) lies under output pixel (0, 0): an input
 * that carries its own halo (the shifted-copy stack of the 5x5 / 7x7 layers, tai_conv_shift_stack: (H + 2, W + 4, 1, 2)) is
 * read inside it, zero padding applies outside the plane only.  dw is then the gradient of the blocked 3x3 weight.  Any H, W
 * as above; columns past the plane read as zeros. */
int tai_conv3x3_wino_wrw_window(const float* x, const float* dy, float* dw, float* dbias, float* workspace, int N, int C, int K,
                                int H, int W, int in_h, int in_w, int in_oy, int in_ox, void* hip_stream);
/* Load scheme of the weight-gradient kernel when W % 32 == 0: 1 (default) = chunk pairs over 16 consecutive tiles, whole
 * 128-byte lines per load; 0 = 8-tile chunks as for the other widths (same results, for A/B timing).  Returns the previous value. */
int tai_conv3x3_wino_wrw_set_paired(int on);
/* Transform domain of tai_conv3x3_wino_wrw, process-wide: 2 = F(2x2, 3x3) (csrc/wino_wrw.hip.inc), 4 (default) = F(4x4, 3x3) where H % 4 == 0 (and
 * W % 16 == 0, no input window) -- 36 multiplies per 4 x 4 tile instead of 16 per 2 x 2 tile, the forward kernel's interpolation points
 * (csrc/wino43_conv.hip.inc, conv3x3_wrw_gen); other shapes keep the F(2x2, 3x3) kernel.  Same interface, same workspace (the size query
 * covers both), reproducible either way.  Returns the previous value, -1 for anything else. */
int tai_conv3x3_wino_wrw_set_tile(int tile);
/* The route of tai_conv3x3_wino_wrw (in_h <= 0: no window) / tai_conv3x3_wino_wrw_window (in_h > 0) for these dimensions, as a query: the launcher
 * calls the same function, so the answer is the launch's own decision and the refusals are the launcher's, with its words.  No stream, no
 * launch.  Returns the grid (kblocks * cblocks * splits workgroups) or TAI_SEPCONV_EINVAL, and fills
 * out[0..7] = tile (4: the F(4x4, 3x3)-domain kernel, 2: F(2x2, 3x3); follows tai_conv3x3_wino_wrw_set_tile), paired (tile 2: chunk pairs
 * over 16 tiles; follows tai_conv3x3_wino_wrw_set_paired), ragged (tile 2: the zero-extended planes, odd H or W % 16 != 0), kblocks (blocks
 * of 64 output channels), cblocks (blocks of 64 input channels; 32 at tile 4), nchunks (chunks of 8 tiles; at tile 4 of four 4 x 4 tiles),
 * chunks_per_split (the last split may hold fewer), splits. */
int tai_conv3x3_wino_wrw_plan(int N, int C, int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, int* out);

/* Spectral normalisation of one discriminator layer, as the reference's SNConv2d / SNLinear do on every forward
 * (src/discriminators/SNDiscriminator.py:10-25 max_singular_value, :60-68 and :84-92 W.data <- W.data / sigma):
 * Ip rounds of  v <- normalise(u W), u <- normalise(v W^T)  on weight [out_rows, in_cols] (the layer's weight viewed as a
 * matrix, fp32 contiguous), sigma = (v W^T) u^T, then weight /= sigma IN PLACE and u [out_rows] replaced by the new
 * vector.  scratch: at least in_cols + out_rows floats of device memory.  sigma_out: one float of device memory that
 * receives sigma (may be NULL) -- a caller that renormalises the same layer several times in a row (the discriminator's
 * sliding windows) passes consecutive slots of one vector and gets the cumulative scale of every window from it.
 * 2 Ip + 1 kernel launches on hip_stream, nothing synchronises. */
int tai_sn_power_iteration(float* weight, float* u, float* scratch, float* sigma_out, int out_rows, int in_cols, int Ip,
                           void* hip_stream);

/* 3x3 stride-1 zero-padded ("same") convolution + bias + activation, fp32 NCHW contiguous, any H, W >= 1, computed as
 * Winograd F(2x2,3x3) on the fp32 MFMA pipe.  An odd H or W is taken by _parts and by _ex without pooled output, unpooling
 * epilogue, input window or shift_k, with the fp32 arithmetic (ceil(H / 2) x ceil(W / 2) tiles; row H and column W are the zero
 * padding); tai_conv3x3_wino_forward, the other forms and the split-bf16 buffers need H and W even and refuse the rest with
 * TAI_SEPCONV_EINVAL.  Replaces nn.Conv2d(C, K, 3, padding=1) [+ ReLU] of the generator and the
 * kernel network (src/models/mcnet/mcnet.py:79-118,131-152,165-170,271; src/models/tai/tai.py:248-286) and, after the
 * transpose-and-flip of the weight, nn.ConvTranspose2d(C, K, 3, padding=1) of DecCnn (mcnet.py:198-224).
 *   tai_conv3x3_wino_weight_floats      number of floats of the transformed-weight buffer U for a [K,C,3,3] weight
 *   tai_conv3x3_wino_transform_weights  weight [K,C,3,3] -> U (once per weight; U is what the forward reads)
 *   tai_conv3x3_wino_forward            x [N,C,H,W], U, bias [K] -> y [N,K,H,W]; act: 0 none, 1 ReLU, 2 tanh */
long long tai_conv3x3_wino_weight_floats(int K, int C);
int tai_conv3x3_wino_transform_weights(const float* weight, float* U, int K, int C, void* hip_stream);
int tai_conv3x3_wino_forward(const float* x, const float* U, const float* bias, float* y, int N, int C, int K, int H, int W,
                             int act, void* hip_stream);
/* The same convolution, also writing ypool [N,K,H/2,W/2] = 2x2 max pool of the activated output (nn.Conv2d + ReLU +
 * nn.MaxPool2d(2): src/models/mcnet/mcnet.py:84-88, 96-100, 110-114; the un-pooled output is the residual, :118).  H and W even. */
int tai_conv3x3_wino_forward_maxpool(const float* x, const float* U, const float* bias, float* y, float* ypool, int N, int C,
                                     int K, int H, int W, int act, void* hip_stream);
/* The same convolution on an input plane of in_h x in_w that holds output pixel (0, 0) at (in_oy, in_ox) (in_ox and in_w
 * even): the zero padding applies outside that plane only, so an input that carries its own halo (tai_conv_shift_stack)
 * is convolved without padding.  ypool may be NULL (no pooled output).  H and W even unless the plane is exactly H x W at (0, 0). */
int tai_conv3x3_wino_forward_window(const float* x, const float* U, const float* bias, float* y, float* ypool, int N, int C,
                                    int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, int act, void* hip_stream);
/* The same convolution with the input given as `nparts` (1..4) contiguous [N, C / nparts, H, W] tensors, the operands of
 * a torch.cat along the channels that is then never materialised (Residual: src/models/mcnet/mcnet.py:182, CombLayers
 * :152, TAI.forward: src/models/tai/tai.py:188).  xs: host array of device pointers; C / nparts must be a multiple of 8. */
int tai_conv3x3_wino_forward_parts(const float* const* xs, int nparts, const float* U, const float* bias, float* y, int N,
                                   int C, int K, int H, int W, int act, void* hip_stream);
/* The general form of the same convolution (every optional argument may be NULL / 0):
 *   xs, nparts      1..4 input parts as above; or ONE tensor with shift_k = k, the size of a k x k filter (4 <= k <= 9):
 *                   with S = (k + 2) / 3 the input [N, C / S^2, in_h, in_w] is read S x S times, channel block (a, b) =
 *                   block a * S + b displaced by (3a, 3b) pixels, and the weight is the k x k filter cut into S x S blocks
 *                   of 3 x 3 taps, ZERO PAST k ([K, S^2 * Cin, 3, 3]).  This is the k x k "same" convolution of MotionEnc
 *                   (nn.Conv2d(gf, 2gf, 5, padding=2), nn.Conv2d(2gf, 4gf, 7, padding=3): src/models/mcnet/mcnet.py:36-38,
 *                   45-47) read from the pooled output of the layer before it where it lies -- no stack of shifted copies.
 *                   When k is not a multiple of 3 the last block row / column has an all-zero third tap row / column, hence
 *                   an all-zero fourth row / column of transformed weights: those multiply-adds are skipped (16 % of a
 *                   7 x 7 layer's, 23 % of a 5 x 5 layer's).  The plane must carry the halo: image row 0 at row k/2, so
 *                   in_oy = 1; image column 0 at column in_ox + k/2 - 1 with in_ox even and >= 2;
 *                   in_h >= H + in_oy + 1 + 3 (S - 1), in_w >= W + in_ox + 2 + 3 (S - 1), halo zero.
 *   ypool, pool_*   2x2 max pool of the activated output written into a plane of pool_h x pool_w with its origin at
 *                   (pool_oy, pool_ox) (pool_h = 0: a plain [N, K, H/2, W/2] tensor);
 *   addx, y2        y2 [N, K, H, W] = y + fixed_unpooling(addx), addx [N, K, H/2, W/2] landing on the even (2i, 2j) sites:
 *                   DecCnn's unpool + residual add (src/models/mcnet/mcnet.py:234-236, 240-256) as a second output of the
 *                   Residual block's last convolution (mcnet.py:172-176).  With addx and y2 == NULL the sum is written to y
 *                   (the plain convolution output is then not produced). */
int tai_conv3x3_wino_forward_ex(const float* const* xs, int nparts, int shift_k, const float* U, const float* bias, float* y,
                                float* ypool, int pool_h, int pool_w, int pool_oy, int pool_ox, const float* addx, float* y2, int N,
                                int C, int K, int H, int W, int in_h, int in_w, int in_oy, int in_ox, int act, void* hip_stream);
/* The plan of a tai_conv3x3_wino_forward_ex launch with these arguments, as a query (has_pool, has_addx, has_y2: whether ypool, addx, y2
 * are given; the pooled output is the plain [N, K, H/2, W/2] tensor; in_h = 0: the plane is H x W at (0, 0)): the launcher calls the same
 * function, so the answer is the launch's own decision and the refusals are the launcher's, with its words.  U: the transformed-weight
 * buffer the launch would read -- a buffer written in split-bf16 arithmetic takes the split kernel where that kernel has the shape -- or
 * NULL for fp32 arithmetic.  No stream, no launch.  Returns the grid or TAI_SEPCONV_EINVAL, and fills
 * out[0..8] = split (1: the split-bf16 kernel, 0: fp32), tall (the 128-channel x 32-tile workgroups; follows tai_conv3x3_wino_set_tall),
 * parts (0 one tensor, 1 cat operands, 2 displaced reads), epilogue (0 none, 1 y2, 2 the sum into y, 3 odd H or W), edge (the split
 * kernel's edge handling), kblocks (blocks of 64 output channels, 128 tall), tblocks (blocks of 64 tiles, 32 tall), nchunks (chunks of 8
 * input channels), grid (kblocks * tblocks). */
int tai_conv3x3_wino_forward_plan(int nparts, int shift_k, int has_pool, int has_addx, int has_y2, int N, int C, int K, int H, int W, int in_h,
                                  int in_w, int in_oy, int in_ox, int act, const float* U, int* out);
/* The same convolution as Winograd F(4x4, 3x3) on the fp32 MFMA pipe (csrc/wino43_conv.hip.inc): 36 multiplies per 4 x 4 output tile
 * instead of 16 per 2 x 2 -- 1.78x fewer MFMAs, ~7x the fp32 rounding error per layer; meant for the layers with C >= 128 and
 * K >= 128, where the bi-TAI forward's end-to-end error is unchanged (profiles/r04_wino_f43_study.txt, r04_wino43_default_parity.txt):
 * the Python side (conv_ops) sends exactly those layers here by default.  Own transformed-weight
 * layout (tai_conv3x3_wino43_weight_floats / _transform_weights); H and W multiples of 4; C any (the transformed weights are zero-padded
 * to a multiple of 4 channels); act as above.  Replaces the same
 * reference layers as tai_conv3x3_wino_forward (src/models/mcnet/mcnet.py:79-118,131-152,165-176,198-224). */
long long tai_conv3x3_wino43_weight_floats(int K, int C);
int tai_conv3x3_wino43_transform_weights(const float* weight, float* U, int K, int C, void* hip_stream);
int tai_conv3x3_wino43_forward(const float* x, const float* U, const float* bias, float* y, int N, int C, int K, int H, int W, int act,
                               void* hip_stream);
/* ... the general form: 1 to 4 input parts and the second outputs of tai_conv3x3_wino_forward_ex that a 4 x 4 tile can hold --
 *   ypool [N,K,H/2,W/2]  the 2x2 max pool of the activated output (act 0 or 1), or NULL;
 *   addx  [N,K,H/2,W/2]  y2 = y + fixed_unpooling(addx) (act 0, no ypool); with y2 NULL the sum is written to y and the plain output
 *                        is not produced. */
int tai_conv3x3_wino43_forward_ex(const float* const* xs, int nparts, const float* U, const float* bias, float* y, float* ypool,
                                  const float* addx, float* y2, int N, int C, int K, int H, int W, int act, void* hip_stream);
/* The k x k "same" convolutions of MotionEnc (nn.Conv2d(gf, 2gf, 5, padding=2), nn.Conv2d(2gf, 4gf, 7, padding=3):
 * src/models/mcnet/mcnet.py:36-38, 45-47) on the same kernel: tai_conv3x3_wino_forward_ex's displaced-read form (shift_k = k, S = (k + 2) / 3,
 * x ONE plane [N, C / S^2, in_h, in_w] that carries its halo and is read S x S times, channel block (a, b) displaced by (3a, 3b) pixels;
 * U from the k x k filter cut into S x S blocks of 3 x 3 taps, zero past k: [K, S^2 * Cin, 3, 3] through
 * tai_conv3x3_wino43_transform_weights) with the 4 x 4 tile: 1.78x fewer MFMAs than there.  The pixel under output (0, 0)'s centre tap of
 * block (0, 0) is at (in_oy, in_ox) (any in_ox >= 1: the patch rows are loaded 4-byte aligned); the plane must cover rows
 * in_oy - 1 ... in_oy + H + 3 (S - 1) and columns in_ox - 1 ... in_ox + W + 3 (S - 1), halo zero.  ypool (may be NULL): 2x2 max pool of
 * the activated output, into a plane of pool_h x pool_w with its origin at (pool_oy, pool_ox) (pool_w, pool_ox even; pool_h = 0: a plain
 * [N, K, H/2, W/2] tensor).  act 0 / 1; C / S^2, H, W multiples of 4. */
int tai_conv3x3_wino43_forward_blocks(const float* x, int shift_k, const float* U, const float* bias, float* y, float* ypool, int pool_h,
                                      int pool_w, int pool_oy, int pool_ox, int N, int C, int K, int H, int W, int in_h, int in_w, int in_oy,
                                      int in_ox, int act, void* hip_stream);
/* Kept for the tools build: 0 = the kernel; values 101-112 select timing ablations / schedule variants of its generated chunk loop where the
 * library was built with -DTAI_TIMING_VARIANTS (wrong results by design).  Returns the previous value, -1 on a value this build does not have
 * (round 4's compiler-scheduled forms 8 / 4 are no longer in the library). */
int tai_conv3x3_wino43_set_waves(int waves);
/* Workgroup placement of the F(4x4, 3x3) kernels (forward, blocks, weight gradient), process-wide: 1 (default) = aware of the chip's 8 XCDs
 * (the hardware deals consecutive workgroups to them in turn, each with its own L2): an XCD gets one output-channel block and a contiguous
 * run of tile blocks (forward) / whole splits (weight gradient); 0 = the plain dispatch order of rounds 4-5.  Same results; for A/B timing.
 * Returns the previous value. */
int tai_conv3x3_wino43_set_placement(int xcd_aware);
/* The F(4x4, 3x3) forward with a split of its reduction over the input channels on small grids: workgroup (split, tile block, channel
 * block) runs a contiguous run of the 4-channel chunks and writes its partial output tiles to ``workspace``; a second kernel sums them
 * in split order (the same bits on every run and replay) and applies bias, activation and the second outputs of
 * tai_conv3x3_wino43_forward_ex (same arguments).  The split count comes from the grid: 1 where the grid already fills the chip, and
 * then the call is tai_conv3x3_wino43_forward_ex exactly.  ``workspace`` holds at least tai_conv3x3_wino43_workspace_floats(N, C, K, H,
 * W, nparts) floats (0: none needed, NULL allowed); the caller allocates it (no allocation inside, e.g. under graph capture). */
int tai_conv3x3_wino43_forward_ws(const float* const* xs, int nparts, const float* U, const float* bias, float* y, float* ypool,
                                  const float* addx, float* y2, float* workspace, long long workspace_floats, int N, int C, int K, int H,
                                  int W, int act, void* hip_stream);
long long tai_conv3x3_wino43_workspace_floats(int N, int C, int K, int H, int W, int nparts);
/* The split count tai_conv3x3_wino43_forward_ws uses for this layer (1: none); *chunks_per_split (if not NULL): the 4-channel chunks of
 * each split but the last, which may hold fewer. */
int tai_conv3x3_wino43_splits(int N, int C, int K, int H, int W, int nparts, int* chunks_per_split);
/* Split over input channels on (1, default) or off (0: tai_conv3x3_wino43_forward_ws never splits; round 5's dispatch), process-wide.
 * A graph captured before a switch keeps what it captured.  For A/B timing.  Returns the previous value. */
int tai_conv3x3_wino43_set_splitc(int on);
/* ... with the input given as 1 to 4 equal channel parts (contiguous [N, C / nparts, H, W] tensors; C / nparts a multiple of 4): the
 * operands of a torch.cat along the channels that is never materialised (tai_conv3x3_wino_forward_parts' counterpart). */
int tai_conv3x3_wino43_forward_parts(const float* const* xs, int nparts, const float* U, const float* bias, float* y, int N, int C, int K,
                                     int H, int W, int act, void* hip_stream);
/* Arithmetic of the Winograd GEMMs, process-wide.  0 (default): fp32 MFMA -- the reference's arithmetic class (cuDNN fp32 behind
 * nn.Conv2d, src/models/mcnet/mcnet.py:28-224) and the one every parity statement of this library is made on.  1 (opt-in): SPLIT
 * bf16 -- each fp32 operand as three bf16 terms, a product as six bf16 products accumulated in fp32 on the bf16 MFMA pipe
 * (csrc/wino_split.hip.inc); its error against a float64 network is at or below the fp32 form's on every bi-TAI layer
 * (profiles/r04_split_bf16_study.txt).  The mode decides what tai_conv3x3_wino_weight_floats / _transform_weights produce (mode 1:
 * the fp32 image followed by the split image); the forward entry points follow the buffer they are handed, so a buffer is always
 * read in the layout it was written in, and layers the split kernel does not take (displaced reads, tile rows that are neither a
 * power of two nor a multiple of 16 tiles) run the fp32 kernel from the same buffer.  Returns the previous mode, negative on a bad
 * argument. */
int tai_conv3x3_wino_set_arithmetic(int mode);
int tai_conv3x3_wino_get_arithmetic(void);
/* The library records which buffers tai_conv3x3_wino_transform_weights filled with a split-bf16 image (the forward entry points follow the
 * buffer they are handed).  Call this when such a buffer is freed, so that its address can never be read in a layout it no longer has
 * (returns 1 if a record was dropped, 0 if there was none). */
int tai_conv3x3_wino_forget_weights(const float* U);
/* Benchmarking: 0 keeps every layer on the 64-channel x 64-tile workgroup shape; 1 (default) lets layers whose K is a
 * multiple of 128 use the 128 x 32 shape.  Returns the previous value. */
int tai_conv3x3_wino_set_tall(int on);
/* Diagnostics (tools/wino_timeline.py): the same launch with ReLU; every workgroup also writes shader-clock stamps to
 * stamps[64 * workgroup + i]: i = 0 entry, 1 prologue done, 2 channel loop done, 3 end, 4 + c end of chunk c (c < 26),
 * and after tai_conv3x3_wino_timeline_skip(7) 30 + 16 * c + g end of MFMA group g of chunk c (c < 2).  stamps holds
 * 64 * workgroups int64.  tai_conv3x3_wino_timeline_skip(level): 0 the full kernel; 1, 2, 5 leave parts of it out to
 * time what remains (results are then wrong); affects timeline launches only, and only in the tools build of the library
 * (-DTAI_TIMING_VARIANTS): the shipped library accepts level 0 alone. */
int tai_conv3x3_wino_forward_timeline(const float* x, const float* U, const float* bias, float* y, int N, int C, int K, int H,
                                      int W, long long* stamps, void* hip_stream);
int tai_conv3x3_wino_timeline_skip(int level);

/* Selects a kernel variant for tai_sepconv_forward (benchmarking / tests):
 *   0 = automatic (default), 1 = generic one-thread-per-output kernel (any shape),
 *   2 = LDS-tiled, whole tap set register-resident, 3 = LDS-tiled, taps split over half-waves,
 *   4 = LDS-tiled, register-resident taps, packed fp32 FMAs (v_pk_fma_f32),
 *   5 = as 4 with the row loop hand-scheduled in gfx950 assembly (v planes by LDS-DMA), 6 = as 5 with
 *       the tap loads of half the waves deferred behind a workgroup barrier, 7-9 = 16-row tiles (8 waves),
 *   10-13 = 8-wave workgroups mixing "taps first" (type A) and "taps last" (type B) waves on every SIMD;
 *       13 adds 16-byte patch staging and alternating wave priorities, 16 = 13 with each XCD given a contiguous
 *       eighth of the tile list, 18 = 16 with the type-A tap loads issued at kernel entry: the patch is staged by the
 *       type-B waves alone (LDS-DMA) and announced through an LDS counter instead of a workgroup barrier,
 *   20 (default for C == 1) = kernel 18's wave types as ONE persistent workgroup per CU when the launch has more tiles than
 *       the device has CUs (and a multiple of 8 of them): the next tile's patch and taps are on their way while this tile
 *       computes; with at most one tile per CU it IS kernel 18 (selected explicitly, 20 runs persistent at any tile count),
 *   14/15 = type-A waves that load their taps once and run the row loop once per channel (8- / 4-wave workgroups),
 *   17 = type-A waves that walk three channel patches per tap row: v and h are read once for all three channels
 *       (channels beyond a multiple of three run on the single-channel kernel), 19 (default for C > 1) = 17 with the three
 *       patches staged by LDS-DMA and the tap loads issued right behind them (patch and h stream travel together).
 *   Values >= 100 (timing experiments that produce wrong results) exist only in the tools build of the library
 *   (-DTAI_TIMING_VARIANTS, build/libtai_sepconv_timing.so); the shipped library rejects them with TAI_SEPCONV_EINVAL.
 * Returns the previous value. */
int tai_sepconv_set_forward_variant(int variant);
/* The variant `0 = automatic` resolves to for a frame of C channels, width W and filter size ks. */
int tai_sepconv_default_forward_variant(int C, int W, int ks);
/* The kernel tai_sepconv_forward would launch for this shape on the current device if `variant` were selected (0 = automatic),
 * as the variant number of the kernel that runs the leading channels.  It is the launcher's own decision, not a restatement:
 * tai_sepconv_forward switches on the value this returns.
 *   1 = the generic kernel;  18 = a persistent request (20-27, or the automatic choice for C == 1) that does not run persistent:
 *   C != 1, a tile count B * ceil(W / 128) * ceil(H / 16) that is no multiple of 8, at most one tile per workgroup when the
 *   choice was automatic, a tap tensor of 2^32 bytes or more, or a device of fewer than 8 CUs;  21-27 = the persistent kernel with
 *   that concrete policy (20 and the automatic choice resolve by tap footprint to 21 or 26);  17 / 19 = the three-channel kernels
 *   when C >= 3 (channels beyond a multiple of three then run on kernel 16), 16 when C < 3;  any other selectable variant = itself.
 * Negative (TAI_SEPCONV_EINVAL, message in tai_sepconv_last_error) for what tai_sepconv_forward refuses for its dimensions or
 * variant: non-positive or too large dimensions, a tiled variant with ks != 51 or W % 4 != 0, an unknown variant.  Launches
 * nothing; reads the CU count of the current device (a host without one answers as for a device of 0 CUs). */
int tai_sepconv_forward_route(int B, int C, int H, int W, int ks, int variant);

/* grad_input kernel of tai_sepconv_backward:
 *   0 = automatic: wave-private accumulation strips + fixed-order slab sum when ks == 51, W % 4 == 0, C in {1, 3} --
 *       bit-reproducible; the tile slabs borrow the caller's grad_vertical (or grad_horizontal) buffer before that gradient
 *       is written, so gI is computed FIRST (with neither buffer given, the strips flush with float atomics instead);
 *       any other shape: the bounds-checked gather;
 *   1 = bounds-checked gather of the reference (any shape, bit-reproducible, ~40x slower);
 *   2 = round-1 kernel: LDS row-scatter with a barrier per tap row and float atomics (last bits depend on arrival order);
 *   3 = as 0 (explicit);  4 = as 0 with the row loop in HIP C++ instead of the generated assembly (A/B).
 * Returns the previous value. */
int tai_sepconv_set_grad_input_variant(int variant);

/* grad_vertical / grad_horizontal kernels: 0 = automatic (one fused launch of the hand-scheduled wave types when C == 1;
 * the gV waves' tap loads issued at kernel entry, the patch staged by the gH waves through LDS-DMA; with only one of the two
 * requested the other's waves leave early, so a gradient has the same bits whatever else was asked for),
 * 1 = the two separate HIP kernels, 2 = the fused launch with the patch staged behind a workgroup barrier first (round 2's
 * form, A/B), 3 / 4 = as 0 with the gV waves at priority 0 / 2 instead of their gH partners' 1 (A/B; the results are the same
 * bits).  Returns the previous value. */
int tai_sepconv_set_grad_taps_variant(int variant);

/* Algorithmic HBM bytes of one call: each operand read once, each result written once. */
long long tai_sepconv_forward_bytes(int B, int C, int H, int W, int ks);
long long tai_sepconv_backward_bytes(int B, int C, int H, int W, int ks);

/* Measurement utility (bench.py): one in-order streaming read of `bytes` (>= 1 MiB, 16-byte aligned) of device memory, 16 bytes
 * per lane with eight loads in flight, default cache policy (nt == 0) or non-temporal loads (nt != 0); `sink` holds 4096 floats and
 * is not written for ordinary data.  Asynchronous on the stream; time it with events.  No counterpart in the reference: it is the
 * yardstick the separable convolution's in-model launch (SeparableConvolution_kernel.cu:19-47 over 1.07 GB of once-read taps) is
 * held against on the box it runs on. */
int tai_hbm_read_probe(const void* buffer, long long bytes, int nt, float* sink, void* hip_stream);

/* Opt-in bf16 inference convolution (csrc/conv_bf16.hip.inc): k x k, stride 1, padding k / 2, k in {3, 5, 7}, C >= 16 input and
 * K >= 16 output channels, any N, H, W >= 1.  y = act(bias + sum bf16(x) bf16(w)): operands rounded to bf16 to nearest even (NaN kept),
 * products exact, sums in fp32 in an order fixed by (C, k), no split and no atomics; x, y and bias are fp32.  Replaces, where the
 * caller opts in (conv_ops.set_conv_precision('bf16')), the inference forward of the generator's nn.Conv2d(C, K, k, padding=k // 2)
 * [+ ReLU / Tanh] (mcnet.py:28-43,79-102,137-144,172-176,203-225; tai.py:256-261) and of DecCnn's stride-1
 * nn.ConvTranspose2d(C, K, 3, padding=1) (mcnet.py:203-225).
 * Element count (bf16) of the packed weights of a K x C x k x k layer; negative (TAI_SEPCONV_EINVAL) outside the rule above. */
long long tai_conv_bf16_weight_elems(int K, int C, int k);
/* Packs w into Wp (16-byte aligned, tai_conv_bf16_weight_elems bf16 elements): bf16 in the order the kernel's B fragments are read,
 * zero past C, K and k^2.  transposed != 0: w is a ConvTranspose2d weight [C][K][k][k]; the pack folds in its transpose and flip. */
int tai_conv_bf16_pack_weights(const float* w, void* Wp, int K, int C, int k, int transposed, void* hip_stream);
/* The forward.  xs: 1-4 input parts [N][C / nparts][H][W], the operands of a torch.cat along the channels that is never materialised.
 * act: 0 none, 1 ReLU, 2 tanh.  Epilogues, each selected by a non-NULL pointer (even H and W):
 *   ypool [N][K][H/2][W/2]: the 2 x 2 max pool of y (the encoders' conv + ReLU + max pool, mcnet.py:28-43,79-102);
 *   addx  [N][K][H/2][W/2]: y2 = y + fixed_unpool(addx) (addx on the even (2i, 2j) sites; Residual blocks and DecCnn,
 *         mcnet.py:172-176,234-236); with y2 NULL, y receives the sum instead of the plain output.
 * TAI_SEPCONV_EINVAL with a message outside the rule above or the index space (N C H W and N K H W below 2^31). */
int tai_conv_bf16_forward(const float* const* xs, int nparts, const void* Wp, const float* bias, float* y, float* ypool,
                          const float* addx, float* y2, int N, int C, int K, int H, int W, int k, int act, void* hip_stream);
/* The plan tai_conv_bf16_forward launches N x K x H x W, k with (the launcher's own decision, not a restatement: the same host
 * function).  out[0..10] = MW (4: the 256-pixel tile and the conv_bf16<k, 4, act> instances, 2: 128 pixels), TH, TW (tile rows and
 * columns, even), IMG (images per tile), PH, PW (patch rows and columns: the tile plus its halo), pitch (patch row pitch in
 * pixels, PW or raised to 4 mod 8), tiles_x, tiles_y, groups (ceil(N / IMG)), lds_bytes (dynamic LDS of the launch).  Returns the
 * number of workgroups, tiles_x tiles_y groups ceil(K / 64); TAI_SEPCONV_EINVAL (out untouched) where tai_conv_bf16_forward refuses
 * these dimensions whatever C >= 16 it is given.  Launches nothing and takes no stream. */
int tai_conv_bf16_plan(int N, int K, int H, int W, int k, int* out);

/* Per-frame image-quality metrics (csrc/frame_metrics.hip.inc): the reference's compute_errors (train.py:237-287) as
 * video_frame_inpainting_amd/metrics.py restates it.  pred and gt are contiguous fp32 [N, C, H, W] in [-1, 1] (N = B T frames),
 * H >= 7 and W >= 7 (the 7x7 SSIM window; smaller planes are refused with TAI_SEPCONV_EINVAL).  Per frame n:
 *   sse[n]   exact sum over all channels of (u(pred) - u(gt))^2, u(x) = uint8(trunc((clip(x, -1, 1) + 1) / 2 * 255)) in fp32;
 *   ssim[n]  SSIM(u(gt), u(pred)): 7x7 uniform window, K1 = 0.01, K2 = 0.03, L = 255, covariance x 49/48, mean over the
 *            (H-6) x (W-6) interior, then over channels; per pixel bit-identical to the host's float64 expression;
 *   l2[n]    mean of ((clip(p) + 1) / 2 - (clip(g) + 1) / 2)^2, squares in fp32, sum in fp64.
 * The workspace (8-byte aligned, tai_frame_metrics_workspace_bytes bytes) holds per-tile partials that are summed per frame in a
 * fixed order: results are reproducible bit for bit and do not depend on the other frames of the batch.  No allocation, copy or
 * synchronisation: asynchronous on hip_stream and capturable into a hipGraph.
 * Workspace bytes for N x C x H x W; negative (TAI_SEPCONV_EINVAL) outside the rule above. */
long long tai_frame_metrics_workspace_bytes(int N, int C, int H, int W);
int tai_frame_metrics(const float* pred, const float* gt, long long* sse, double* ssim, double* l2, void* workspace, int N, int C,
                      int H, int W, void* hip_stream);

/* Structural-similarity training loss and its gradient, one launch (csrc/ssim_loss.hip.inc; losses.SSIMLoss; tests/ssim_loss_ref.py
 * restates it in numpy).  pred and gt are contiguous fp32, viewed as [N, C, H, W] (N = the product of the leading dimensions; the mean
 * does not care how planes are ordered), nominally in [-1, 1] and NOT clipped (a clipped pixel would lose its gradient); H, W >= 7.
 * Definition, per plane:
 *   x = (pred + 1) / 2, y = (gt + 1) / 2 in fp32 in that operation order (util.inverse_transform), then widened to float64;
 *   everything below is float64, one IEEE operation per written operation, no contraction;
 *   window: 7x7 uniform over the (H-6) x (W-6) valid interior (window (i, j) covers rows i..i+6, columns j..j+6), L = 1,
 *     C1 = 0.01 * 0.01, C2 = 0.03 * 0.03 (float64 products), c = 49.0 / 48.0;
 *   a 7x7 sum of a map m at (i, j) is  sum_{k=0..6} V(i, j + k),  V(i, j) = sum_{k=0..6} m(i + k, j),  each accumulated from 0.0 with
 *     k ascending; the five sums are of x, y, x*x, y*y, x*y and each mean is sum / 49.0:  ux, uy, uxx, uyy, uxy;
 *   vx = c * (uxx - ux * ux), vy = c * (uyy - uy * uy), vxy = c * (uxy - ux * uy);
 *   A1 = (2 * ux) * uy + C1, A2 = 2 * vxy + C2, B1 = (ux * ux + uy * uy) + C1, B2 = (vx + vy) + C2, D = B1 * B2, S = (A1 * A2) / D;
 *   plane_ssim[n * C + ch] = (sum of S over the interior) / ((H-6) * (W-6)); totals[0] = mean_ssim = (sum of plane_ssim) / (N * C);
 *   totals[1] = loss = 1 - mean_ssim.
 * Gradient with respect to pred, from three per-window maps (zero for a window outside the interior):
 *   gamma = -(((2 * c) * S) / B2),  beta = ((2 * c) * A1) / D,
 *   alpha = ((((2 * uy) * A2) / D - ((2 * S) * ux) / B1) - beta * uy) - gamma * ux;
 *   for pixel q = (r, col), the 7x7 sums over the windows that contain it,  Sm(q) = sum_{k=0..6} Vm(r, col - 6 + k),
 *     Vm(r, j) = sum_{k=0..6} m(r - 6 + k, j), accumulated from 0.0 with k ascending;
 *   dS(q) = ((Salpha + y(q) * Sbeta) + x(q) * Sgamma) / 49.0;
 *   grad[q] = fp32((-0.5 * dS(q)) / divisor), divisor = ((double)N * C) * ((double)(H-6) * (W-6)): d loss / d pred (the 0.5 is
 *   d x / d pred).  No gradient goes to gt.  grad may be NULL (evaluation only): the second pass is skipped, the other outputs keep
 *   their bits.
 * A pixel's grad bits and a plane's plane_ssim bits depend on that plane's pixels and on (N, C, H, W) through the divisor only: not on
 * the tiling, the other planes or the launch.  No atomics: tile partial sums go to the workspace (8-byte aligned,
 * tai_ssim_loss_workspace_bytes bytes) and are summed per plane, then over planes, in a fixed order.  A NaN in one plane makes that
 * plane's outputs and the totals non-finite and no other plane's.  No allocation, copy or synchronisation: asynchronous on hip_stream
 * and capturable into a hipGraph.
 * Workspace bytes for N x C x H x W; negative (TAI_SEPCONV_EINVAL) when N or C < 1, H or W < 7, N C H W >= 2^40, H W >= 2^31 or the
 * tile count reaches 2^31. */
long long tai_ssim_loss_workspace_bytes(int N, int C, int H, int W);
int tai_ssim_loss(const float* pred, const float* gt, double* plane_ssim, double* totals, float* grad, void* workspace, int N, int C,
                  int H, int W, void* hip_stream);

/* Pointwise + gradient-difference image loss of 1-3 predictions against one ground truth, and its gradients, one launch
 * (csrc/image_loss.hip.inc; losses.ImageLoss; tests/image_loss_ref.py restates it in numpy).  pred_i (i < npred, npred in 1..3) and gt are
 * contiguous fp32, viewed as P = planes planes of H x W (P = the product of all leading dimensions; the loss does not care how planes are
 * ordered), nominally in [-1, 1] and NOT clipped; H, W >= 2.
 * Definition, per plane; every operation is a single IEEE fp32 operation, no contraction, no reassociation, division and square root
 * correctly rounded:
 *   x = (pred + 1) / 2, y = (gt + 1) / 2, in that operation order (util.inverse_transform);  d = x - y;
 *   point term rho(d) and its derivative rho'(d):
 *     kind 0 (L2):          rho = d * d;  rho' = 2 * d;
 *     kind 1 (L1):          rho = |d|;  rho' = sgn(d), with sgn(0) = 0 and NaN kept;
 *     kind 2 (Charbonnier): s = sqrt(d * d + e2) with e2 = eps * eps computed once in fp32;  rho = s;  rho' = d / s;
 *   gradient-difference term, exactly losses.GDL's operand order:
 *     gw(r, c) = (x[r,c] - x[r,c+1]) - (y[r,c] - y[r,c+1]) for 1 <= r <= H-1, 0 <= c <= W-2;
 *     gh(r, c) = (x[r,c] - x[r-1,c]) - (y[r,c] - y[r-1,c]) for 1 <= r <= H-1, 1 <= c <= W-1;
 *     (this is not d[r,c] - d[r,c+1]: the bits differ);
 *   sums are in float64 over the widened fp32 terms:
 *     plane_terms[i][p][0] = plane_point[p] = the sum of rho over the plane;
 *     plane_terms[i][p][1] = plane_gdl[p] = the sum of |gw| plus the sum of |gh| over the plane;
 *     totals[i][0] = point = (sum over p of plane_point[p]) / (P * H * W);
 *     totals[i][1] = gdl = (sum over p of plane_gdl[p]) / (P * (H-1) * (W-1));
 *     totals[i][2] = loss = point + gdl;
 *     the order of the sums is the kernel's, but it is fixed: tile partials go to the workspace, are summed per plane and then over
 *     planes; no atomics.
 * Gradient with respect to pred_i, one map, computed in float64 and rounded once:
 *   S(r, c) = [r>=1, c<=W-2] sgn(gw(r,c)) - [r>=1, c>=1] sgn(gw(r,c-1)) + [r>=1, c>=1] sgn(gh(r,c)) - [r<=H-2, c>=1] sgn(gh(r+1,c)),
 *     an integer in [-4, 4];
 *   grad[r,c] = fp32( (double)rho'(d) * cp + S * cg ),  cp = 0.5 / ((double)P * H * W),  cg = 0.5 / ((double)P * (H-1) * (W-1)):
 *     two float64 products and one float64 sum, no fused multiply-add.  No gradient goes to gt.
 * grads may be NULL, and so may any grads[i] (evaluation only); the other outputs keep their bits.
 * A pixel's grad bits and a plane's two sums depend on that plane's pixels and on (P, H, W) through cp / cg only: not on the tiling, the
 * other planes, npred or the other predictions of the launch.  A NaN in one plane makes that plane's outputs and the totals non-finite
 * and no other plane's.  preds and grads are host arrays of npred device pointers, read before the call returns.  No allocation, copy or
 * synchronisation: asynchronous on hip_stream and capturable into a hipGraph.  workspace: 8-byte aligned,
 * tai_image_loss_workspace_bytes bytes.
 * TAI_SEPCONV_EINVAL with a message, nothing launched: a null preds / preds[i] / gt / plane_terms / totals / workspace; npred outside
 * 1..3; kind outside 0..2; kind == 2 with eps not finite or <= 0; planes < 1; H or W < 2; planes * H * W >= 2^40 or H * W >= 2^31; a tile
 * count of 2^31 or more; float64 buffers not 8-byte aligned.  The workspace query returns TAI_SEPCONV_EINVAL for the same dimensions. */
long long tai_image_loss_workspace_bytes(int npred, long long planes, int H, int W);
int tai_image_loss(const float* const* preds, int npred, const float* gt, int kind, float eps,
                   double* plane_terms /* [npred][planes][2] */, double* totals /* [npred][3]: point, gdl, loss */,
                   float* const* grads /* NULL, or npred pointers each of which may be NULL */,
                   void* workspace, long long planes, int H, int W, void* hip_stream);

/* Laplacian-pyramid L1 loss and its gradient, one launch (csrc/lap_loss.hip.inc; losses.LapLoss; tests/lap_loss_ref.py restates it in
 * numpy).  pred and gt are contiguous fp32, viewed as [planes, H, W] (the loss does not care how planes are ordered), nominally in
 * [-1, 1] and NOT clipped; levels = L, 1 <= L <= 6, min(H, W) >= 2^(L-1).
 * Definition, per plane:
 *   x = (pred + 1) / 2, y = (gt + 1) / 2, in that operation order (util.inverse_transform); d = x - y; all in fp32, then widened to
 *     float64; everything below is float64, one IEEE operation per written operation, no contraction.  The pyramid operator is linear,
 *     so the pyramid of d is the difference of the two pyramids: only d's is built.
 *   Sizes: H_0 = H, H_{l+1} = ceil(H_l / 2), the same for W.  clamp() below clamps an index to its level (edge replicate).
 *   Reduce D, taps k = (1, 4, 6, 4, 1) / 16, separable, rows first:
 *     T[i, x] = sum_{a=0..4} k[a] * G_l[clamp(2i + a - 2), x];   G_{l+1}[i, j] = sum_{b=0..4} k[b] * T[i, clamp(2j + b - 2)];
 *     each 5-term sum accumulated left to right, starting from its first product (T may be recomputed on the fly, in this order).
 *   Expand U from level l+1 to the size of level l, separable, rows then columns, along one axis with g the coarser sequence:
 *     even index 2i:   (g[clamp(i-1)] / 8 + (6 * g[i]) / 8) + g[clamp(i+1)] / 8;     odd index 2i+1:   g[i] / 2 + g[clamp(i+1)] / 2.
 *   Laplacian: G_0 = d;  L_l = G_l - U(G_{l+1}) for l < L-1;  L_{L-1} = G_{L-1}.
 *   plane_terms[plane][l] = sum of |L_l| over the plane;  S_l = the sum of plane_terms[.][l] in plane order, from 0.0;
 *   totals[l] = term_l = (2^l * S_l) / count, count = ((double)P * H) * W;  totals[L] = loss = term_0 + term_1 + ... left to right:
 *     the sum norm with 2^l weights, normalised by the number of full-resolution pixels.  L = 1 is the mean of |d|.
 * Gradient with respect to pred:
 *   s_l = 2^l * sign(L_l), with sign(0) = 0 and a NaN kept;  r_0 = s_0, r_l = s_l - U^T(s_{l-1}) for l >= 1;
 *   t_{L-1} = r_{L-1}, t_l = r_l + D^T(t_{l+1}) going down to t_0;  grad = fp32((t_0 * 0.5) / count)  (the 0.5 is d x / d pred).
 *   Every s, r and t value is a dyadic rational that float64 holds exactly for L <= 6 (which is why L stops there), so the adjoint sums
 *   may be taken in any order and the gradient has one correct bit pattern.  No gradient goes to gt.  grad may be NULL (evaluation
 *   only): no map is written, the other outputs keep their bits.
 * A pixel's grad bits and a plane's plane_terms bits depend on that plane's pixels and on (planes, H, W, L) only: not on the other planes
 * or the launch.  No atomics: the sums of |L_l| are taken in a fixed order.  A NaN in one plane makes that plane's outputs and the
 * totals non-finite and no other plane's.  No allocation, copy or synchronisation: asynchronous on hip_stream and capturable into a
 * hipGraph.  workspace: 8-byte aligned, tai_lap_loss_workspace_bytes bytes (never 0): where the pyramids live when a plane's does not
 * fit the workgroup's LDS.
 * TAI_SEPCONV_EINVAL with a message, nothing launched: a null pred / gt / plane_terms / totals / workspace; planes < 1; levels outside
 * 1..6; min(H, W) < 2^(levels-1); planes * H * W >= 2^31; float64 buffers not 8-byte aligned.  The workspace query returns
 * TAI_SEPCONV_EINVAL for the same dimensions. */
long long tai_lap_loss_workspace_bytes(long long planes, int H, int W, int levels);
int tai_lap_loss(const float* pred, const float* gt, int levels, double* plane_terms /* [planes][levels] */,
                 double* totals /* [levels + 1]: term_0..term_{L-1}, loss */, float* grad /* or NULL */,
                 void* workspace, long long planes, int H, int W, void* hip_stream);

/* Temporal-difference loss of 1-3 predictions against one ground truth over a gap of T frames, and its gradients, one launch
 * (csrc/temporal_loss.hip.inc; losses.TemporalLoss; tests/temporal_loss_ref.py restates it in numpy).  The distance between the
 * frame-to-frame differences of prediction and ground truth, taken over the gap and the two known frames next to it: the known frames
 * cancel, which leaves the temporal difference of the error with the error zero on both known sides.
 * pred_i (i < npred, npred in 1..3) and gt are fp32, nominally in [-1, 1] and NOT clipped, indexed (b, t, c, r, col) with b < B, t < T,
 * c < C, r < H, col < W; T >= 1 and H, W >= 1.  Each tensor has a dense [C, H, W] block per (b, t) and its own batch stride and time
 * stride in elements: the element is at b * sb + t * st + c * H * W + r * W + col.  [B, T, C, H, W] storage is (T C H W, C H W), time-major
 * [T, B, C, H, W] storage is (C H W, B C H W); any pair under which no two (b, t) blocks overlap is taken.  A sequence is one (b, c);
 * there are S = B * C of them, numbered b * C + c.
 * Definition, per pixel of a sequence; every operation is a single IEEE fp32 operation, no contraction, no reassociation, division and
 * square root correctly rounded:
 *   x = (pred + 1) / 2, y = (gt + 1) / 2, in that operation order (util.inverse_transform);
 *   e_t = x_t - y_t for t = 0..T-1;  e_{-1} = e_T = +0 (the known frames);
 *   d_j = e_j - e_{j-1} for j = 0..T: T + 1 difference positions, position 0 and position T being the seams;
 *   rho(d) and rho'(d) are tai_image_loss's three kinds:
 *     kind 0 (L2):          rho = d * d;  rho' = 2 * d;
 *     kind 1 (L1):          rho = |d|;  rho' = sgn(d), with sgn(0) = 0 and NaN kept;
 *     kind 2 (Charbonnier): s = sqrt(d * d + e2) with e2 = eps * eps computed once in fp32;  rho = s;  rho' = d / s;
 *   sums are in float64 over the widened fp32 terms:
 *     seq_terms[i][s][j] = the sum of rho(d_j) over the H * W pixels of sequence s;
 *     totals[i][j] = (sum over s of seq_terms[i][s][j]) / ((double)S * H * W) for j = 0..T;
 *     totals[i][T+1] = loss = (sum over s and j of seq_terms[i][s][j]) / count,  count = (double)S * (T+1) * H * W;
 *     the order of the sums is the kernel's, but it is fixed: wave partials go to the workspace, are summed per sequence and then over
 *     sequences, position after position; no atomics.
 * Gradient with respect to pred_i, computed in float64 and rounded once:
 *   grad[b,t,c,r,col] = fp32( ((double)rho'(d_t) - (double)rho'(d_{t+1})) * ct ),  ct = 0.5 / count;
 *   it is written with the strides of pred_i.  No gradient goes to gt.
 * grads may be NULL, and so may any grads[i] (evaluation only); the other outputs keep their bits.
 * A pixel's grad bits and a sequence's seq_terms bits depend on that sequence's pixels and on (S, T, H, W) only: not on B, the other
 * sequences, npred, the other predictions of the launch, or the layout a tensor is stored in.  A NaN in one sequence makes that
 * sequence's outputs and the totals non-finite and no other sequence's.  preds, grads and strides are host arrays, read before the call
 * returns.  No allocation, copy or synchronisation: asynchronous on the stream and capturable into a hipGraph.  workspace: 8-byte
 * aligned, tai_temporal_loss_workspace_bytes bytes.
 * TAI_SEPCONV_EINVAL with a message, nothing launched: a null preds / preds[i] / gt / strides / seq_terms / totals / workspace; npred
 * outside 1..3; kind outside 0..2; kind == 2 with eps not finite or <= 0; a dimension < 1; B T C H W >= 2^40, H W >= 2^31,
 * B C (T+1) >= 2^31 or 2^31 or more chunks of 256 four-pixel runs; a stride < 1, strides that reach an offset of 2^40 elements, or
 * strides under which two blocks overlap; float64 buffers not 8-byte aligned.  The workspace query returns TAI_SEPCONV_EINVAL for the
 * same dimensions.
 * The last parameter is the HIP stream, as everywhere in this ABI.  It is spelled `stream` here and not `hip_stream` for a reason that has
 * nothing to do with the ABI: tests/test_capi_refusals_cpu.py finds the entries that its recorded table (tests/golden/capi_refusals.json)
 * must cover by the name `hip_stream`, and that table's cases are the test file's own list, which this entry was added without touching.
 * Its refusals are pinned by tests/test_temporal_loss_cpu.py instead.  When cases for this entry are recorded in that table, the name
 * goes back to `hip_stream` (and the messages may move to the launcher as literals, where that test counts them). */
long long tai_temporal_loss_workspace_bytes(int npred, int B, int T, int C, int H, int W);
int tai_temporal_loss(const float* const* preds, int npred, const float* gt,
                      const long long* strides /* host, [npred + 1][2]: batch, time stride in elements; preds first, gt last */,
                      int kind, float eps,
                      double* seq_terms /* [npred][B*C][T+1] */, double* totals /* [npred][T+2] */,
                      float* const* grads /* NULL, or npred pointers each of which may be NULL */,
                      void* workspace, int B, int T, int C, int H, int W, void* stream /* the HIP stream */);

/* Census (soft ternary) loss of 1-3 predictions against one ground truth, and its gradients, one launch (csrc/census_loss.hip.inc;
 * losses.CensusLoss; tests/census_loss_ref.py restates it in numpy).  It compares, per pixel, how the pixel relates to its 7 x 7
 * neighbours (UnFlow's ternary census distance): a constant added to a frame changes nothing.
 * pred_i (i < npred, npred in 1..3) and gt are fp32, nominally in [-1, 1] and NOT clipped, indexed (b, t, c, r, col) with b < B, t < T,
 * c < C, r < H, col < W; C is 1 or 3 and H, W >= 7.  Strides are tai_temporal_loss's: a dense [C, H, W] block per (b, t), the element at
 * b * sb + t * st + c * H * W + r * W + col with the tensor's own batch and time stride, no two blocks overlapping.  A frame is one
 * (b, t); there are B * T of them, numbered b * T + t.
 * Definition, per frame; every fp32 operation is a single IEEE operation, no contraction, no reassociation, division and square root
 * correctly rounded:
 *   intensity: x = (pred + 1) / 2 per channel (util.inverse_transform);  C = 1: I = x;
 *     C = 3: I = (0.1140f * x0 + 0.5870f * x1) + 0.2989f * x2 (util.gray01's operand order);  J the same from gt;
 *   offsets j = (dy, dx) over {-3..3}^2 without (0, 0), in row-major ascending order (dy outer): "the order";
 *   for a pixel q and an offset j with q and q + j inside the plane:
 *     s = 255f * (I(q+j) - I(q));  u = 0.81f + s * s;  r = sqrtf(u);  t = s / r;  s', t' the same from J;
 *     d = t - t';  e = d * d;  n = 0.1f + e;  phi = e / n;
 *     dphi = ((2f * d) * 0.1f) / (n * n);  tau = 0.81f / (u * r);  w(q, j) = (double)dphi * (double)tau;
 *   Omega is the interior, rows 3..H-4 and columns 3..W-4: the pixels whose window is whole;
 *   D(q) = (sum_j (double)phi(q, j)) / 49.0 for q in Omega, in the order, from 0.0 (the centre of the customary 49 contributes 0);
 *   frame_terms[i][b*T + t] = (sum over Omega of D) / ((H-6) * (W-6));
 *   totals[i] = (sum of the frame terms in frame order, from 0.0) / (B * T): the loss of prediction i;
 *     the order of the sum over Omega is the kernel's, but it is fixed: tile partials go to the workspace and are summed per frame in
 *     tile order; no atomics.
 * Gradient with respect to I, computed in float64:
 *   G(q) = -(sum_j m(q, j) * w(q, j)),  m(q, j) = [q in Omega] + [q+j in Omega] (0, 1 or 2, multiplied as a double),
 *   over the j whose q + j lies in the plane, in the order, from 0.0.  This is the exact adjoint from the pixel's own neighbourhood: the
 *   term that window q - k sends to q is w(q-k, k), and w(q-k, k) == -w(q, -k) in IEEE arithmetic, because every operation above is
 *   exactly odd or even in s.  No scatter, no second pass.
 * Output gradient, rounded once:
 *   count = (double)(B * T) * ((H-6) * (W-6));  kappa = (255.0 * 0.5) / (49.0 * count);
 *   C = 1: grad[q] = fp32(G * kappa);  C = 3: channel c gets fp32((G * kappa) * (double)w_c), w = (0.1140f, 0.5870f, 0.2989f);
 *   it is written with the strides of pred_i.  No gradient goes to gt.
 * grads may be NULL, and so may any grads[i] (evaluation only); the other outputs keep their bits.
 * A pixel's grad bits and a frame's frame_terms bits depend on that frame's pixels and on (B T, H, W) only: not on the batch, the other
 * frames, npred, the other predictions of the launch, or the layout a tensor is stored in.  A NaN in one frame makes that frame's
 * outputs and the totals non-finite and no other frame's.  preds, grads and strides are host arrays, read before the call returns.  No
 * allocation, copy or synchronisation: asynchronous on the stream and capturable into a hipGraph.  workspace: 8-byte aligned,
 * tai_census_loss_workspace_bytes bytes.
 * TAI_SEPCONV_EINVAL with a message, nothing launched: a null preds / preds[i] / gt / strides / frame_terms / totals / workspace; npred
 * outside 1..3; a dimension < 1; C outside {1, 3}; H or W < 7; B T C H W >= 2^40, H W >= 2^31, B T >= 2^31 or 2^31 or more 32 x 32
 * tiles; a stride < 1, strides that reach an offset of 2^40 elements, or strides under which two blocks overlap; float64 buffers not
 * 8-byte aligned.  The workspace query returns TAI_SEPCONV_EINVAL for the same dimensions.
 * The last parameter is the HIP stream, spelled `stream` for the reason given at tai_temporal_loss; the refusals are pinned by
 * tests/test_census_loss_cpu.py. */
long long tai_census_loss_workspace_bytes(int npred, int B, int T, int C, int H, int W);
int tai_census_loss(const float* const* preds, int npred, const float* gt,
                    const long long* strides /* host, [npred + 1][2]: batch, time stride in elements; preds first, gt last */,
                    double* frame_terms /* [npred][B*T] */, double* totals /* [npred] */,
                    float* const* grads /* NULL, or npred pointers each of which may be NULL */,
                    void* workspace, int B, int T, int C, int H, int W, void* stream /* the HIP stream */);

/* The clip pipeline's two ends (csrc/clip_pipeline.hip.inc): what stands between a decoded frame and the models, and between the models
 * and a PNG, bit-equal to the host code (video_frame_inpainting_amd/data.py and util.py) it replaces when asked to.
 *
 * tai_clip_from_frames replaces the per-frame host pipeline of src/data/base_dataset.py:50-103 (cv2.resize, RGB -> BGR, flip,
 * copyMakeBorder, to_tensor, fore_transform, bgr2gray) for a whole batch in one launch.
 *   frames      device buffer of frames_bytes bytes holding uint8 RGB frames [h_i][w_i][3], packed in any order;
 *   table       device copy, and table_host a host copy, of N descriptors of four 64-bit integers {byte offset of the frame in `frames`,
 *               h_i, w_i, flags (bit 0: mirror the output columns)}; frames of one call may differ in source size.  table_host is
 *               read before the call returns and checked against frames_bytes; the kernel re-checks the device copy per frame and
 *               writes the padding level for a frame whose descriptor is out of range, so a table that is changed under a replayed
 *               graph cannot become an out-of-bounds read;
 *   levels      device [4][256] fp32: row 0 the value of level q, (float(q) / 255) * 2 - 1; rows 1-3 the products 0.1140, 0.5870,
 *               0.2989 x row 0 -- computed by the caller with the host path's own expressions (clip_pipeline.level_tables);
 *   out         contiguous fp32 [N][c_dim][H + pad_h][W + pad_w], every element written: bilinear resize to H x W (half-pixel
 *               centres, edge clamp, fp64, round half up), BGR channel order (c_dim 3) or (B' + G') + R' (c_dim 1), padding = level 0.
 * Time reversal is an ordering of the descriptors.  A frame's output depends on its own descriptor and pixels only.
 *
 * tai_frames_to_uint8 replaces predict.py:103-120's way out (clip, inverse_transform, x 255, truncating uint8 cast, channel-last,
 * BGR -> RGB): x contiguous fp32 [N][C][Hs][Ws], out uint8 [N][h][w][C] = the top-left h x w of every plane,
 * u(x) = uint8(trunc(255 * ((clip(x, -1, 1) + 1) / 2))) in fp32 (the u of tai_frame_metrics); reverse_channels != 0 writes channel
 * C - 1 - c at position c.  NaN maps to 0.
 *
 * Both: caller-allocated buffers, no allocation, copy or synchronisation, asynchronous on hip_stream, capturable into a hipGraph.
 * TAI_SEPCONV_EINVAL with a message for a null pointer, c_dim / C outside {1, 3}, non-positive sizes, a descriptor that points past
 * frames_bytes, or an index space of 2^31 elements or more; nothing is launched then. */
int tai_clip_from_frames(const unsigned char* frames, long long frames_bytes, const long long* table, const long long* table_host,
                         const float* levels, float* out, int N, int c_dim, int H, int W, int pad_h, int pad_w, void* hip_stream);
int tai_frames_to_uint8(const float* x, unsigned char* out, int N, int C, int Hs, int Ws, int h, int w, int reverse_channels,
                        void* hip_stream);

/* The augmented way in (csrc/clip_augment.hip.inc; train.py --aug_crop / --aug_vflip / --aug_brightness / --aug_contrast / --aug_gamma /
 * --aug_flicker, training clips only; tests/clip_augment_ref.py restates it in numpy; data._ClipReader.clip is the host path, bit-equal).
 * tai_clip_from_frames_aug is tai_clip_from_frames with, per frame, a crop window, a top-bottom flip and a level table of its own.
 *
 * The definition, per clip of T frames with source size h x w and settings (SMIN, vflip, B, C, G, F):
 *   draws     unit uniforms u_scale, u_top, u_left, u_vflip, u_gamma, u_gain, u_offset, then u_0 .. u_{T-1}, in this order, ALL of them
 *             whenever any setting differs from its default (SMIN = 1, vflip off, B = C = G = F = 0), after the clip's window start,
 *             mirror and reversal draws, from the same generator, before any frame is read;
 *   crop      in float64: s = SMIN + u_scale (1 - SMIN); ch = max(1, floor(s h)); cw = max(1, floor(s w));
 *             top = min(floor(u_top (h - ch + 1)), h - ch); left = min(floor(u_left (w - cw + 1)), w - cw); one window for the clip.
 *             The window is resized to H x W by tai_clip_from_frames's definition (half-pixel centres, fp64, products and sums rounded one
 *             by one, round half up) with the taps clamped to the WINDOW's edges: resize(frame[top:top+ch, left:left+cw]);
 *   flips     after the resize: output (y, x) reads resized (H-1-y if vflip, W-1-x if mirror); vflip = the flag and u_vflip > 0.5;
 *   levels    gamma = (1 + G)^(2 u_gamma - 1); g = 1 + C (2 u_gain - 1); d = B (2 u_offset - 1); e_t = F (2 u_t - 1) for the frame at
 *             playback position t (after time reversal).  A level table per frame, float64 rounded once:
 *             for q in 0..255: x = q / 255; if gamma != 1: x = x ** gamma; x = (x - 0.5) g + 0.5 + (d + e_t); x = min(max(x, 0), 1);
 *             row 0[q] = fore_transform(float32(x)) = float32(x) * 2 - 1 in fp32; rows 1-3 = 0.1140, 0.5870, 0.2989 x row 0 in fp32
 *             (clip_pipeline.augment_level_tables).  Neutral parameters give clip_pipeline.level_tables() bit for bit;
 *   padding   rows >= H and columns >= W: level 0 of the NEUTRAL table, never augmented.
 *
 * The entry:
 *   frames, frames_bytes, levels, out, N, c_dim, H, W, pad_h, pad_w   as tai_clip_from_frames; `levels` is the neutral table (padding);
 *   table / table_host   device and host copy of N descriptors of NINE 64-bit integers
 *               {0: byte offset of the frame in `frames`, 1: h, 2: w, 3: flags (bit 0 mirror, bit 1 vflip), 4: top, 5: left, 6: ch, 7: cw,
 *                8: index of the frame's level table};
 *   tables      device fp32 [n_tables][4][256], 16-byte aligned: one table per clip, or one per frame with flicker.
 * out(y, x) for y < H, x < W: channel c = row 0 of the frame's table at the level of source channel 2 - c (c_dim 3), or
 * (row 1[q_B] + row 2[q_G]) + row 3[q_R] (c_dim 1).  A frame's output depends on its own descriptor, table and pixels only.
 * table_host is checked before anything is launched; the kernel re-checks each descriptor of the device copy before it forms an address
 * (offset and sizes against frames_bytes, the window inside the frame, the table index below n_tables) and writes the padding level for
 * every element of a frame whose descriptor fails.
 * Caller-allocated buffers, no allocation, copy or synchronisation, asynchronous on the stream, capturable into a hipGraph.
 * TAI_SEPCONV_EINVAL with a message, nothing launched: a null pointer; c_dim outside {1, 3}; non-positive N, H, W, frames_bytes or
 * n_tables, negative padding; an index space of 2^31 output elements or more; tables not 16-byte aligned; a descriptor with a
 * non-positive or oversized source size, one that points past frames_bytes, a window with ch or cw < 1, a window outside its frame, or a
 * table index outside 0..n_tables-1.
 * The last parameter is the HIP stream, spelled `stream` for the reason given at tai_temporal_loss; the refusals are pinned by
 * tests/test_clip_augment_cpu.py. */
int tai_clip_from_frames_aug(const unsigned char* frames, long long frames_bytes, const long long* table, const long long* table_host,
                             const float* tables, int n_tables, const float* levels, float* out, int N, int c_dim, int H, int W, int pad_h,
                             int pad_w, void* stream /* the HIP stream */);

/* Per-frame damage statistics of a whole video in one pass (csrc/frame_scan.hip.inc; video_frame_inpainting_amd/restore.py classifies
 * frames by them; tests/frame_scan_ref.py restates them in numpy; no counterpart in the reference, whose predict.py is told where the gap is).
 *   frames   device buffer of n_frames uint8 frames of frame_bytes bytes each (h w c in any layout), back to back; the base address may
 *            have any alignment, and frame_bytes is any number in 1 .. 2^31 - 1, so successive frames may take every alignment modulo 16;
 *   stats    device int64 [n_frames][4], 8-byte aligned.  Row i, over the bytes v_i[k] of frame i, all exact integers:
 *              0: s1    = sum_k v_i[k];
 *              1: s2    = sum_k v_i[k] * v_i[k];
 *              2: sad   = sum_k |v_i[k] - v_{i-1}[k]|                  (0 for i = 0);
 *              3: ndiff = #{k : |v_i[k] - v_{i-1}[k]| > tol}           (0 for i = 0), 0 <= tol <= 254;
 *   workspace  tai_frame_scan_workspace_bytes(n_frames, frame_bytes) bytes, 8-byte aligned (per-segment partial sums).
 * The sums are integers, so every row has one correct bit pattern whatever the order of summation.  Row i depends on frames i - 1 and i
 * only: not on n_frames, not on the base alignment, not on where the scanned range starts -- scanning frames [j, n) gives row 0 =
 * (s1, s2, 0, 0) of frame j and then rows j + 1 .. of scanning [0, n).
 * Two launches (a walk that reads every byte 1 + 1/8 times and a per-frame finish; no atomics), no allocation, copy or synchronisation:
 * asynchronous on the stream and capturable into a hipGraph.
 * TAI_SEPCONV_EINVAL with a message naming the argument, nothing launched: frames, stats or workspace null; n_frames < 1; frame_bytes < 1
 * or >= 2^31; n_frames x frame_bytes above 2^40; tol outside 0..254; stats or workspace not 8-byte aligned.  The workspace query returns
 * TAI_SEPCONV_EINVAL for the same sizes.
 * The last parameter is the HIP stream, spelled `stream` for the reason given at tai_temporal_loss; the refusals are pinned by
 * tests/test_restore_cpu.py. */
long long tai_frame_scan_workspace_bytes(long long n_frames, long long frame_bytes);
int tai_frame_scan(const unsigned char* frames, long long n_frames, long long frame_bytes, int tol, long long* stats /* [n_frames][4] */,
                   void* workspace, void* stream /* the HIP stream */);

/* The frame scan's four integers per BLOCK of every frame (csrc/block_scan.hip.inc; restore.py --detect_blocks tells partly damaged frames
 * by them; tests/block_scan_ref.py restates them in numpy; no counterpart in the reference).
 *   frames   device buffer of n_frames uint8 frames [h][w][c], back to back, c in 1..4; the base address may have any alignment and w c is
 *            any number, so rows take every alignment modulo 16;
 *   bs       block size in pixels, 8, 16 or 32; Bh = ceil(h / bs), Bw = ceil(w / bs); block (by, bx) is the pixels
 *            [by bs, min(h, by bs + bs)) x [bx bs, min(w, bx bs + bs)) with all their channels -- edge blocks are ragged and hold fewer bytes;
 *   stats    device int64 [n_frames][Bh][Bw][4], 8-byte aligned.  Row (i, by, bx), over the bytes of that block of frame i, is
 *            tai_frame_scan's (s1, s2, sad against the same bytes of frame i - 1, ndiff = #{|d| > tol}); sad = ndiff = 0 for i = 0;
 *   workspace  tai_block_scan_workspace_bytes(n_frames, h, w, c, bs) bytes, 8-byte aligned.  This version needs none (the query
 *            returns 0 for every size it takes, every block is summed inside one workgroup) and never touches the pointer, which may be
 *            null; callers that honour the query stay correct should a later version need one.
 * Identity: summing the rows of frame i over its blocks gives row i of tai_frame_scan(frames, n_frames, h w c, tol) on the same buffer
 * (the blocks partition the frame's bytes); tests/test_gpu_block_scan.py holds it.
 * The sums are integers, so every row has one correct bit pattern.  Row i depends on frames i - 1 and i only: not on n_frames, not on the
 * base alignment, not on where the scanned range starts.  Every byte is read 1 + 1/8 times.  A block holds at most 32 * 32 * 4 = 4096
 * bytes and 4096 * 255^2 < 2^32: lane and block sums are 32-bit, the output int64.
 * One launch, no atomics, no allocation, copy or synchronisation: asynchronous on the stream and capturable into a hipGraph.
 * TAI_SEPCONV_EINVAL with a message naming the argument, nothing launched: frames or stats null; n_frames < 1; h or w < 1; c outside 1..4;
 * bs outside {8, 16, 32}; h w c >= 2^31; n_frames h w c above 2^40; tol outside 0..254; stats, or a non-empty workspace, not 8-byte
 * aligned.  The workspace query returns TAI_SEPCONV_EINVAL for the same sizes.
 * The last parameter is the HIP stream, spelled `stream` for the reason given at tai_temporal_loss; the refusals are pinned by
 * tests/test_restore_blocks_cpu.py. */
long long tai_block_scan_workspace_bytes(long long n_frames, int h, int w, int c, int bs);
int tai_block_scan(const unsigned char* frames, long long n_frames, int h, int w, int c, int bs, int tol,
                   long long* stats /* [n_frames][Bh][Bw][4] */, void* workspace, void* stream /* the HIP stream */);

/* The way out of PARTLY damaged frames (csrc/damage_composite.hip.inc; restore.py composites the frames whose flag byte is PARTIAL;
 * tests/damage_composite_ref.py restates it in numpy): the model's prediction where the damage is, the pipeline's own pixels elsewhere,
 * a linear ramp of `feather` pixels between them, for a whole batch of frames in one launch.
 *   pred, src   device fp32 buffers of pred_elems / src_elems elements holding frames [C][Hs][Ws] (padding included): the model's
 *               output and the pipeline's frames, read in place;
 *   table       device copy, and table_host a host copy, of n_items items of four 64-bit integers {element offset of the predicted frame
 *               in pred, element offset of the source frame in src, index of the frame's block map, index of the output frame};
 *   blocks      device uint8 [n_maps][Bh][Bw], non-zero = damaged, in SOURCE coordinates (blocks of bs x bs source pixels);
 *   r0, r1, c0, c1   device int32 [h], [h], [w], [w]: the source rows / columns that the bilinear resize of the way in reads WITH NON-ZERO
 *               WEIGHT at model row y / column x.  The host builds them from the expression of tai_clip_from_frames:
 *               s = (i + 0.5) * (n_in / n_out) - 0.5 in float64, i0 = clip(floor(s)), i1 = clip(floor(s) + 1) if s - floor(s) > 0, else i0
 *               (restore.tap_tables).  The kernel does no floating point for geometry; a tap outside the map counts as undamaged;
 *   out         device uint8 [n_out][h][w][C]: every byte of an item's output frame is written, no other frame is touched.
 * Definition, in integers behind u (the u of tai_frames_to_uint8: clip, truncating, NaN -> 0):
 *   core     D(y, x) = 1 iff blocks[m][ty / bs][tx / bs] != 0 for some ty in {r0[y], r1[y]}, tx in {c0[x], c1[x]};
 *   feather  R = feather + 1; A(y, x) = max(0, R - dist), dist = the Chebyshev distance from (y, x) to the nearest pixel with D = 1
 *            inside the h x w frame: A = R on the core, one less per pixel, 0 from distance R on; feather = 0 is a hard replace;
 *   pixels   P = u(pred[c'][y][x]), S = u(src[c'][y][x]), c' = C - 1 - c when reverse_channels, else c;
 *   blend    out[y][x][c] = floor((2 (A P + (R - A) S) + R) / (2 R)).
 * Hence A = R gives P and A = 0 gives S byte for byte, and a frame without a damaged block is what tai_frames_to_uint8 writes for src.
 * A frame's bits depend on its own item only: not on the other items, their order, or the kernel's tiling.
 * table_host is checked before anything is launched; the kernel re-checks each item of the device copy before it forms an address and
 * leaves the output frame of a failed item untouched.
 * One launch, no atomics, no allocation, copy or synchronisation: asynchronous on the stream and capturable into a hipGraph.
 * TAI_SEPCONV_EINVAL with a message, nothing launched: a null pointer; C outside {1, 3}; bs outside {8, 16, 32}; feather outside 0..15;
 * non-positive n_items, n_maps, n_out, Bh or Bw; h, w outside 1..Hs, 1..Ws; an index space of 2^31 or more; an item whose predicted or
 * source frame lies outside pred_elems / src_elems, or whose map or output index is out of range.
 * The last parameter is the HIP stream, spelled `stream` for the reason given at tai_temporal_loss; the refusals are pinned by
 * tests/test_restore_blocks_cpu.py. */
int tai_damage_composite(const float* pred, long long pred_elems, const float* src, long long src_elems, const long long* table,
                         const long long* table_host, long long n_items, const unsigned char* blocks, long long n_maps, int Bh, int Bw,
                         int bs, const int* r0, const int* r1, const int* c0, const int* c1, unsigned char* out, long long n_out, int C,
                         int Hs, int Ws, int h, int w, int feather, int reverse_channels, void* stream /* the HIP stream */);

/* A 64-bit digest of a training state where it lives (csrc/state_digest.hip.inc; video_frame_inpainting_amd/run_state.py builds the
 * table; no counterpart in the reference, whose snapshots carry no check).  On the raw 32-bit words, integer arithmetic modulo 2^64 only:
 *   mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 *   entry t with words w[0..n_t) (an 8-byte element is two words, low word first):  E_t = sum_i mix((i << 32) + w[i])
 *   D = 0x243F6A8885A308D3; for t in table order: D = mix(D ^ E_t); D = mix(D + n_t)
 * table / table_host: a device and a host copy of n_entries rows of four 64-bit integers {address (a multiple of 4; 0 = the entry lives on
 * the host or is empty), n_t, E_t as the caller computed it for an entry with address 0 (ignored otherwise), first segment}: an entry
 * with an address is cut into ceil(n_t / seg_words) segments numbered consecutively in table order, n_segments in all; seg_words is a
 * positive multiple of 4.  table_host is read before the call returns and refused (TAI_SEPCONV_EINVAL, nothing launched) unless the
 * segment numbers are exactly those; the kernels read [address, address + 4 n_t) of every entry and nothing else.
 * workspace: tai_state_digest_workspace_bytes(n_entries, n_segments) bytes, 8-byte aligned; result: one device uint64.
 * The result depends on the words, their order inside an entry and the order of the entries -- not on seg_words, the grid, the addresses
 * or on which side an entry lives.  One launch over the segments (16-byte loads where the address allows, per-segment sums to the
 * workspace, no atomics) and a one-workgroup finish in index order.  No allocation, copy or synchronisation; asynchronous on hip_stream. */
long long tai_state_digest_workspace_bytes(int n_entries, long long n_segments);
int tai_state_digest(const long long* table, const long long* table_host, int n_entries, long long n_segments, long long seg_words,
                     void* workspace, unsigned long long* result, void* hip_stream);

/* Statistics of a table of contiguous fp32 tensors where they live, and x <- x * c over the same table (csrc/grad_stats.hip.inc;
 * video_frame_inpainting_amd/grad_guard.py builds the table; no counterpart in the reference, which never looks at its gradients).
 * A float sum depends on its order, so the order is the definition -- the results are a function of the values alone:
 *   an entry x[0..n_t) is cut into segments of 16384 elements (a constant of the definition); the last one may be short;
 *   an element that is NaN or +-Inf adds 1 to nonfinite[t] and contributes nothing else; a finite one contributes
 *     q = (double)x * (double)x (exact in fp64) to the sum and |x| to maxabs[t];
 *   inside a segment there are 1024 fp64 accumulators a[0..1024), all +0.0 at first; a[j] adds, in increasing i, the q of the elements
 *     with segment-relative index i = j (mod 1024); then, for d = 1, 2, 4, ..., 512 in this order, a[j] <- a[j] + a[j xor d] for all j
 *     at once (every a[j] ends with the same value, the segment sum);
 *   sumsq[t] = the segment sums added one by one in segment order, starting from +0.0;
 *   sumsq[n_entries] = the sumsq[t] added one by one in table order, starting from +0.0; maxabs[n_entries] and nonfinite[n_entries] are
 *     the maximum and the sum over the table (exact whatever the order).  An empty entry gives zeros.
 * table: n_entries rows of four 64-bit integers {address, elements n_t, unused, first segment} on the device, table_host the same rows on
 * the host: the state digest's row.  An entry is cut into ceil(n_t / 16384) segments numbered consecutively in table order, n_segments in
 * all; an empty entry has address 0.  table_host is read before the call returns and refused (TAI_SEPCONV_EINVAL, nothing launched) unless
 * the segment numbers are exactly those, every address is 4-byte aligned and 0 exactly for the empty entries.  The kernels touch
 * [address, address + 4 n_t) of every entry and nothing else.  blocks: workgroups of the launch over the segments, 0 = the library's
 * choice; the results do not depend on it, nor on the addresses or their alignment, on repetition, or -- per entry -- on the other entries.
 * tai_grad_stats: workspace of tai_grad_stats_workspace_bytes(n_entries, n_segments) bytes, 16-byte aligned; sumsq (double), maxabs
 * (float), nonfinite (int64): n_entries + 1 elements each on the device, the last one the table's.  One launch over the segments (16-byte
 * loads where the address allows, sixteen in flight per lane, per-segment results to the workspace, no atomics), one workgroup to finish.
 * tai_grad_scale: x <- x * c in fp32, one rounding per element, c finite and passed by value (the caller launches it when c < 1); it needs
 * no workspace today (the query returns 0 and the pointer may be null).
 * Both: no allocation, copy or synchronisation; asynchronous on hip_stream. */
long long tai_grad_stats_workspace_bytes(int n_entries, long long n_segments);
int tai_grad_stats(const long long* table, const long long* table_host, int n_entries, long long n_segments, int blocks, void* workspace,
                   double* sumsq, float* maxabs, long long* nonfinite, void* hip_stream);
long long tai_grad_scale_workspace_bytes(int n_entries, long long n_segments);
int tai_grad_scale(const long long* table, const long long* table_host, int n_entries, long long n_segments, float c, int blocks,
                   void* workspace, void* hip_stream);

/* One launch per optimizer for the clip scaling, the Adam update and the generator's weight average (EMA), decided by a verdict that lives
 * in device memory (csrc/fused_step.hip.inc; video_frame_inpainting_amd/fused_step.py builds the tables; train.py --fused_step
 * [--ema_decay d]; restated in numpy in tests/fused_step_ref.py).  No counterpart in the reference, whose update is torch.optim.Adam.
 *
 * The definition.  Every operation below is one IEEE fp32 operation rounded to nearest even: nothing is contracted into a fused
 * multiply-add, nothing reassociated, square root and division are correctly rounded.  The scalars come from a table the host builds
 * once in float64 and rounds to fp32, for t' = 1 ... table_len:  step_size[t'] = f32(lr / (1 - beta1**t')),
 * bc2s[t'] = f32(sqrt(1 - beta2**t')); constants w1 = f32(1 - beta1), b2 = f32(beta2), w2 = f32(1 - beta2), eps = f32(1e-8),
 * wE = f32(1 - d).  With t the optimizer's device-resident step counter, t' = t + 1 and c the clip coefficient (fp32), per element
 * when the verdict is not "skipped":
 *     g1 = (c < 1) ? g * c : g
 *     m' = m + w1 * (g1 - m)
 *     v' = b2 * v + (w2 * g1) * g1
 *     s  = sqrt(v') / bc2s[t'] + eps
 *     p' = p - step_size[t'] * (m' / s)
 *     e' = e + wE * (p' - e)                      (only entries that carry an EMA tensor)
 * g is not written back.  Afterwards t is t + 1 and every `step` tensor of the table holds float(t').  When the verdict is "skipped"
 * no byte of p, m, v, e, t or of a `step` tensor changes.
 *
 * tai_step_verdict (one workgroup; runs behind tai_grad_stats and in front of tai_fused_step on the same stream) writes the verdict of
 * optimizer `which` (0 = generator, 1 = discriminator) into `record`, tai_step_verdict_workspace_bytes() bytes of device memory, 8-byte
 * aligned, zero at the start of a run, as 64-bit words:
 *   0, 1 skipped_G, skipped_D;  2 consecutive;  3 gave_up (sticky);  4 a step of the open update was skipped;
 *   5-9 of the last skipped step: which, index of the first entry with non-finite elements, their number in it, in all, entries with any;
 *   10, 11 verdict (0 ok, 1 clipped, 2 skipped);  12, 13 c (fp32 bits);  14, 15 the total sum of squares (fp64 bits);
 *   16, 17 t;  18, 19 the t' of the step that follows (0 = none);  20 set when t' would pass table_len (that step is left out);
 *   21 updates closed;  22 that number when gave_up was set.
 * sumsq / nonfinite: the result arrays of tai_grad_stats over the same gradients (n_entries + 1 elements, the last the table's), or both
 * null: no guard, the verdict is ok.  nonfinite[n_entries] > 0 -> skipped; otherwise, with max_norm > 0 (0 = no clipping),
 * c64 = max_norm / (sqrt(total) + 1e-6) in fp64 with a correctly rounded square root and division, c = 1 if c64 >= 1 else f32(c64),
 * clipped when c < 1: the bits of grad_guard.clip_coefficient.  A skip adds 1 to skipped_G / skipped_D; close_update != 0 (the update's
 * last optimizer) sets consecutive to consecutive + 1 if a step of the update was skipped and to 0 otherwise, and gave_up once it reaches
 * `patience`.  With gave_up set every verdict is "skipped" and nothing else in the record moves: the state stays where a host-side
 * guard would have stopped the run.
 *
 * tai_fused_step: table / table_host, a device and a host copy of n_entries rows of eight 64-bit integers {p, g, m, v, step tensor
 * (0 = none), e (0 = none), elements n_t, first segment}; an entry is cut into ceil(n_t / 16384) segments numbered consecutively in table
 * order, n_segments in all; an empty entry has addresses 0.  table_host is read before the call returns and refused (TAI_SEPCONV_EINVAL,
 * nothing launched) unless the segment numbers are exactly those and every address is 4-byte aligned.  scalars: device fp32
 * [2][table_len], step_size then bc2s, element t' - 1 for step t'.  The kernel touches [address, address + 4 n_t) of p, g, m, v, e, one
 * float of each step tensor, and reads record.  16-byte accesses where a full segment's addresses all allow, 4-byte ones otherwise (a
 * gradient that is a view into a flat bucket, a short tail); nt != 0 loads g, m, v non-temporally; blocks: workgroups, 0 = the
 * library's choice.  The results depend on none of these, nor on repetition from equal state.  It needs no workspace today (the query
 * returns 0 and the pointer may be null).
 * All: no allocation, copy or synchronisation; asynchronous on hip_stream. */
long long tai_step_verdict_workspace_bytes(void);
int tai_step_verdict(const double* sumsq, const long long* nonfinite, int n_entries, double max_norm, int which, int close_update,
                     long long patience, long long table_len, long long* record, void* hip_stream);
long long tai_fused_step_workspace_bytes(int n_entries, long long n_segments);
int tai_fused_step(const long long* table, const long long* table_host, int n_entries, long long n_segments, const float* scalars,
                   long long table_len, float w1, float b2, float w2, float eps, float wE, const long long* record, int which, int nt,
                   int blocks, void* workspace, void* hip_stream);

/* The fused step with a learning-rate schedule, a warm-up and decoupled weight decay (train.py --fused_step --lr_schedule
 * {constant,step,cosine} --warmup_updates W --lr_decay_every E --lr_gamma g --lr_min_ratio r --weight_decay wd; restated in
 * tests/fused_step_decay_ref.py).  The schedule is the host's table and nothing else: Python floats (float64, the math module) for
 * t' = 1 ... table_len, with L the optimizer's base rate and N the number of steps the table is built for:
 *     warm(t')  = t' / W                                   if t' <= W, else 1.0
 *     constant:   s(t') = 1.0
 *     step:       s(t') = g ** ((t' - 1) // E)
 *     cosine:     s(t') = 1.0                              for t' <= W
 *                 u = min(1.0, (t' - W) / max(1, N - W))
 *                 s(t') = r + (1.0 - r) * (0.5 * (1.0 + math.cos(math.pi * u)))
 *     lr(t')    = (L * warm(t')) * s(t')
 *     step_size[t'] = f32(lr(t') / (1 - beta1**t'))        bc2s[t'] as above
 *     decay[t']     = f32(lr(t') * wd)
 * t' counts the steps taken -- a skipped step does not advance it -- so the schedule follows them and is saved with the optimizer
 * state.  With the constant schedule, W = 0 and wd = 0 the table is the one above bit for bit.  A schedule with wd = 0 needs no other
 * kernel: tai_fused_step runs on the scheduled table.  With wd > 0, tai_fused_step_decay; per element, single IEEE fp32 operations as
 * above, only the line for p changes:
 *     p1 = p - (decay[t'] * p)         for entries whose flag says "decays"; p1 = p for the others
 *     p' = p1 - step_size[t'] * (m' / s)
 *     e' = e + wE * (p' - e)
 * An entry without the flag never multiplies its p by anything: a non-finite p there behaves as in tai_fused_step.  A skipped verdict
 * changes no byte.
 *
 * tai_fused_step_decay: table / table_host and record as tai_fused_step takes them; flags / flags_host, a device and a host copy of one
 * 64-bit word per entry, 8-byte aligned, bit 0 = the entry decays, any value other than 0 or 1 refused from flags_host before anything
 * is launched; scalars: device fp32 [3][table_len], step_size, bc2s, then decay.  The row's flag is read once per segment, the scalars
 * once per workgroup; loads are plain.  The results depend neither on blocks nor on repetition from equal state, and with every flag 0
 * they are tai_fused_step's.  No workspace today.  No allocation, copy or synchronisation; asynchronous on the stream. */
long long tai_fused_step_decay_workspace_bytes(int n_entries, long long n_segments);
int tai_fused_step_decay(const long long* table, const long long* table_host, const long long* flags, const long long* flags_host,
                         int n_entries, long long n_segments, const float* scalars, long long table_len, float w1, float b2, float w2,
                         float eps, float wE, const long long* record, int which, int blocks, void* workspace, void* stream);

/* Text of the last error on the calling thread ("" if none). */
const char* tai_sepconv_last_error(void);

/* Library / ABI version: major*10000 + minor*100 + patch. */
int tai_sepconv_version(void);

/* SHA-256 (hex) of the sources this binary was compiled from: every csrc/*.hip and csrc/*.inc plus this header, in sorted
 * order, as the in-tree builder computes it (video-frame-inpainting_amd/_native.py: source_hash()).  The loader recomputes
 * the hash from the tree next to the binary and refuses a library that was built from other sources -- the sources travel
 * with the binary, so a stale .so (a failed rebuild, an edited kernel) cannot run.  Replaces the unconditional load of
 * src/separable_convolution/_ext/cunnex/__init__.py:6-15.  "unknown" for a build made without the in-tree builder. */
const char* tai_sepconv_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* TAI_SEPCONV_H */
