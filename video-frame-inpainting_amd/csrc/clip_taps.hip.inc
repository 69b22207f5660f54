// The resize arithmetic the clip pipeline's kernels share (included by clip_pipeline.hip.inc, ahead of both from_frames and
// clip_augment.hip.inc's from_frames_aug): `tap` and `blend` as the contract at the head of clip_pipeline.hip.inc states them -- fp64,
// contraction OFF, every product and sum rounded on its own.  Both are __forceinline__, so each kernel carries its own copy.

namespace clip {

struct Tap { int i0, i1; double f; };

__device__ __forceinline__ Tap tap(int i, int n_out, int n_in) {
#pragma clang fp contract(off)
    const double scale = (double)n_in / (double)n_out;
    const double src = ((double)i + 0.5) * scale - 0.5;
    const double fl = floor(src);
    Tap t;
    t.f = src - fl;
    const int i0 = (int)fl;
    t.i0 = min(max(i0, 0), n_in - 1);
    t.i1 = min(max(i0 + 1, 0), n_in - 1);
    return t;
}

__device__ __forceinline__ int blend(const unsigned char* __restrict__ r0, const unsigned char* __restrict__ r1, int xa, int xb, double fx,
                                     double fy) {
#pragma clang fp contract(off)
    const double a = (double)r0[xa], b = (double)r0[xb], c = (double)r1[xa], d = (double)r1[xb];
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const double top = a * gx + b * fx;
    const double bot = c * gx + d * fx;
    const double v = top * gy + bot * fy;
    const double r = floor(v + 0.5);
    return (int)fmin(fmax(r, 0.0), 255.0);
}

}  // namespace clip
