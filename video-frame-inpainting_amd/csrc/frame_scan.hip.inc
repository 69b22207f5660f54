// Per-frame damage statistics of a whole uint8 video in one pass (included by sepconv_capi.hip): what restore.py classifies frames by.
// The definition is the one include/tai_sepconv.h writes down for tai_frame_scan and tests/frame_scan_ref.py restates in numpy.  For
// frame i of n_frames frames of frame_bytes bytes each, back to back, four exact integers:
//   s1 = sum v;  s2 = sum v * v;  sad = sum |v_i - v_{i-1}|;  ndiff = #{ |v_i - v_{i-1}| > tol }   (sad = ndiff = 0 for i = 0).
//
// Exactness: all four are sums of non-negative integers, so they have one correct bit pattern whatever the order.  Row i reads frames
// i - 1 and i and nothing else; the split into segments and runs, the grid and the base alignment only decide who adds what.
//
// Work split: a frame is cut into an unaligned head (0..15 bytes, up to the first 16-byte boundary), whole 16-byte vectors, and a tail
// (0..15 bytes).  A work item is one segment of THREADS vectors (one per lane, SEG_BYTES in all) crossed with a run of RUN consecutive
// frames.  The lane issues the loads of its vector in all RUN frames and in the frame before the run up front (RUN + 1 loads of 16 bytes
// in flight per lane, 36 KiB per workgroup), then walks the run with the previous frame's vector in registers: every byte of the video is
// read 1 + 1 / RUN times, not twice.  The head and tail bytes (at most 30 per frame) are walked the same way, one byte per lane, by the first
// lanes of segment 0.  RUN = 8: a 128 x 128 gray video of 512 frames is 4 segments x 64 runs = 256 work items, one for each compute unit.
//
// Alignment: when frame_bytes is a multiple of 16 every frame has the base's alignment, the head is chosen so that every vector is
// 16-byte aligned, and all of them are read with 16-byte loads (the ALIGNED instance: no branch at a load).  Otherwise successive frames
// take different alignments, the vectors start at the frame's first byte (no head, the tail is frame_bytes % 16) and each is read with
// the widest loads its address allows: 16 bytes, four words, or single bytes (load16; the address's low bits are the same for all lanes of
// a workgroup, so the branch is uniform).  Each has an instance for tol = 0, the default, whose count of differing bytes is cheaper.
//
// Accumulators: a lane adds at most LANE_BYTES = 17 bytes per frame (its vector and one edge byte) into 32-bit registers:
// 17 * 255 * 255 = 1,105,425 < 2^32, so not even s2 at all-255 input can overflow; the four sums of the 256 lanes go through LDS as
// 32-bit words and are added in 64 bits (256 * 1,105,425 < 2^29 would fit 32 bits as well).  The workgroup's four sums of frame f and
// segment s go to the workspace, [n_frames][segments][4]; `finish` adds a frame's segments, one wave per frame.  No atomics.  Both grids
// are capped at GRID_CAP workgroups; past it a workgroup strides.

#include "loss_common.hip.inc"

namespace fscan {

constexpr int THREADS = 256;
constexpr int RUN = 8;                                 // frames per work item
constexpr int VEC_BYTES = 16;
constexpr long long SEG_BYTES = THREADS * VEC_BYTES;   // bytes of one frame a work item covers
constexpr int LANE_BYTES = VEC_BYTES + 1;              // per frame: the lane's vector and one head / tail byte
constexpr long long GRID_CAP = 1LL << 14;
constexpr int STATS = 4;                               // s1, s2, sad, ndiff
constexpr long long MAX_TOTAL_BYTES = 1LL << 40;       // n_frames * frame_bytes: every byte offset and workspace index stays below 2^47

static_assert((unsigned long long)LANE_BYTES * 255 * 255 < (1ULL << 32), "a lane's 32-bit accumulators hold its bytes at all-255 input");
static_assert(RUN * STATS * 8 == THREADS, "the LDS reduction gives each (frame of the run, statistic) eight threads");

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

struct Args {
    const unsigned char* frames;
    long long* part;               // [n_frames][nseg][STATS]
    long long n_frames, frame_bytes;
    long long nvec;                // whole vectors of a frame
    long long nseg;                // ceil(nvec / THREADS), at least 1 (the edge bytes ride on segment 0)
    long long items;               // nseg * ceil(n_frames / RUN)
    int head, tail;                // bytes in front of / behind the vectors, 0..15 each
    int tol;
};

// 16 bytes at q with the widest loads the address allows (the not-ALIGNED instance)
__device__ __forceinline__ uint4 load16(const unsigned char* q) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(q);
    if ((a & 15) == 0) return *reinterpret_cast<const uint4*>(q);
    uint4 v;
    if ((a & 3) == 0) {
        // volatile: the compiler may not merge these with the 16-byte load of the other branch, nor move them out of theirs
        const volatile unsigned* w = reinterpret_cast<const volatile unsigned*>(q);
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    } else {
        const volatile unsigned char* b = q;
        unsigned d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            d[k] = (unsigned)b[4 * k] | ((unsigned)b[4 * k + 1] << 8) | ((unsigned)b[4 * k + 2] << 16) | ((unsigned)b[4 * k + 3] << 24);
        v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
    }
    return v;
}

// four bytes x of a frame against the same bytes p of the frame before it
template <bool TOL0>
__device__ __forceinline__ void add_word(unsigned x, unsigned p, unsigned tol2, us2 tolv, unsigned& s1, unsigned& s2, unsigned& sad,
                                         unsigned& nd) {
    s1 = __builtin_amdgcn_sad_u8(x, 0u, s1);                 // sum of the four bytes
    s2 = __builtin_amdgcn_udot4(x, x, s2, false);            // sum of their squares
    sad = __builtin_amdgcn_sad_u8(x, p, sad);                // sum of the four absolute differences
    if (TOL0) {
        // tol = 0 (the default: exact repeats) counts the bytes that differ at all: the non-zero bytes of x ^ p.  Adding 0x7F to a
        // byte's low seven bits carries into its bit 7 exactly when one of them is set, and never into the next byte
        const unsigned y = x ^ p;
        nd += (unsigned)__builtin_popcount((((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u);
        return;
    }
    // |x - p| > tol per byte, two bytes at a time in 16-bit halves: w = x - p + tol wraps below zero to >= 65281, so
    // |x - p| <= tol  <=>  w <= 2 tol as an unsigned 16-bit number
#pragma unroll
    for (int odd = 0; odd < 2; ++odd) {
        const unsigned xe = (x >> (8 * odd)) & 0x00FF00FFu, pe = (p >> (8 * odd)) & 0x00FF00FFu;
        const us2 w = __builtin_bit_cast(us2, xe) - __builtin_bit_cast(us2, pe) + tolv;
        nd += (unsigned)(w.x > tol2) + (unsigned)(w.y > tol2);
    }
}

template <bool ALIGNED, bool TOL0>
__global__ __launch_bounds__(THREADS)
void walk(const Args a) {
    __shared__ unsigned lane_sums[RUN * STATS][THREADS];
    const int t = threadIdx.x;
    const long long n = a.n_frames, fb = a.frame_bytes;
    const unsigned tol2 = 2u * (unsigned)a.tol;
    const us2 tolv = {(unsigned short)a.tol, (unsigned short)a.tol};
    const int n_edge = a.head + a.tail;
    // the edge byte of lane t < n_edge: head byte t, or tail byte t - head behind the vectors
    const long long edge_off = t < a.head ? t : (long long)a.head + a.nvec * VEC_BYTES + (t - a.head);

    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long r = item / a.nseg, s = item - r * a.nseg;
        const long long f0 = r * RUN;                                        // the run's first frame
        const int nf = (int)(n - f0 < RUN ? n - f0 : RUN);                   // its frames, 1..RUN
        const long long vec = s * THREADS + t;
        const bool live = vec < a.nvec;
        const bool edge = s == 0 && t < n_edge;
        const long long off = a.head + vec * VEC_BYTES;                      // + 16 <= head + 16 nvec <= frame_bytes when live

        // slot j holds frame f0 - 1 + j: slot 0 is the frame before the run (absent for the first run, never used then)
        uint4 v[RUN + 1];
        unsigned e[RUN + 1];
#pragma unroll
        for (int j = 0; j <= RUN; ++j) {
            const long long f = f0 - 1 + j;
            const bool there = f >= 0 && j <= nf;
            v[j] = make_uint4(0u, 0u, 0u, 0u);
            e[j] = 0u;
            if (there && live) {
                const unsigned char* q = a.frames + f * fb + off;
                v[j] = ALIGNED ? *reinterpret_cast<const uint4*>(q) : load16(q);
            }
            if (there && edge) e[j] = a.frames[f * fb + edge_off];
        }

#pragma unroll
        for (int j = 1; j <= RUN; ++j) {
            unsigned s1 = 0u, s2 = 0u, sad = 0u, nd = 0u;
            if (j <= nf) {
                add_word<TOL0>(v[j].x, v[j - 1].x, tol2, tolv, s1, s2, sad, nd);
                add_word<TOL0>(v[j].y, v[j - 1].y, tol2, tolv, s1, s2, sad, nd);
                add_word<TOL0>(v[j].z, v[j - 1].z, tol2, tolv, s1, s2, sad, nd);
                add_word<TOL0>(v[j].w, v[j - 1].w, tol2, tolv, s1, s2, sad, nd);
                const unsigned d = e[j] > e[j - 1] ? e[j] - e[j - 1] : e[j - 1] - e[j];
                s1 += e[j];
                s2 += e[j] * e[j];
                sad += d;
                nd += (unsigned)(d > (unsigned)a.tol);
                if (f0 == 0 && j == 1) { sad = 0u; nd = 0u; }                // frame 0 has no frame before it
            }
            lane_sums[(j - 1) * STATS + 0][t] = s1;
            lane_sums[(j - 1) * STATS + 1][t] = s2;
            lane_sums[(j - 1) * STATS + 2][t] = sad;
            lane_sums[(j - 1) * STATS + 3][t] = nd;
        }
        __syncthreads();

        // eight threads per (frame of the run, statistic): each adds 32 lanes' words, rotated by its own index so that the threads of a
        // wave read different banks, in 64 bits; the eight are neighbours in a wave
        {
            const int k = t >> 3, piece = t & 7;
            long long acc = 0;
#pragma unroll 8
            for (int i = 0; i < 32; ++i) acc += (long long)lane_sums[k][piece * 32 + ((i + t) & 31)];
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            const int j = k / STATS, q = k - j * STATS;
            if (piece == 0 && j < nf) a.part[((f0 + j) * a.nseg + s) * STATS + q] = acc;
        }
        __syncthreads();          // the sums are read before the next item writes them
    }
}

// One wave per frame: its lanes add the frame's segments, a butterfly adds the lanes.
__global__ __launch_bounds__(THREADS)
void finish(const long long* __restrict__ part, long long* __restrict__ stats, long long n_frames, long long nseg) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long f = (long long)blockIdx.x * (THREADS / 64) + wave; f < n_frames; f += (long long)gridDim.x * (THREADS / 64)) {
        long long acc[STATS] = {0, 0, 0, 0};
        for (long long s = lane; s < nseg; s += 64) {
            const long long* q = part + (f * nseg + s) * STATS;
#pragma unroll
            for (int k = 0; k < STATS; ++k) acc[k] += q[k];
        }
#pragma unroll
        for (int k = 0; k < STATS; ++k) acc[k] = losscommon::wave_sum(acc[k]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < STATS; ++k) stats[f * STATS + k] = acc[k];
        }
    }
}

// what tai_frame_scan and its workspace query refuse for the sizes; null: they are taken
inline const char* refusal(long long n_frames, long long frame_bytes) {
    if (n_frames < 1) return "frame_scan: n_frames must be >= 1";
    if (frame_bytes < 1 || frame_bytes >= (1LL << 31)) return "frame_scan: frame_bytes must be >= 1 and below 2^31";
    if (n_frames > MAX_TOTAL_BYTES / frame_bytes) return "frame_scan: n_frames x frame_bytes must not exceed 2^40";
    return nullptr;
}

// everything tai_frame_scan refuses, before any runtime call; null: the launch goes ahead
inline const char* call_refusal(const unsigned char* frames, long long n_frames, long long frame_bytes, int tol, const long long* stats,
                                const void* workspace) {
    if (!frames) return "frame_scan: frames is a null pointer";
    if (!stats) return "frame_scan: stats is a null pointer";
    if (!workspace) return "frame_scan: workspace is a null pointer";
    if (const char* why = refusal(n_frames, frame_bytes)) return why;
    if (tol < 0 || tol > 254) return "frame_scan: tol must be in 0..254";
    if (reinterpret_cast<uintptr_t>(stats) % 8 || reinterpret_cast<uintptr_t>(workspace) % 8)
        return "frame_scan: stats and workspace must be 8-byte aligned";
    return nullptr;
}

// the cut of a frame at base alignment `base_mod16` (taken sizes only)
inline Args plan(long long n_frames, long long frame_bytes, int base_mod16) {
    Args a = {};
    a.n_frames = n_frames;
    a.frame_bytes = frame_bytes;
    a.head = frame_bytes % VEC_BYTES == 0 ? (VEC_BYTES - base_mod16) % VEC_BYTES : 0;     // < frame_bytes: that is >= 16 then
    a.nvec = (frame_bytes - a.head) / VEC_BYTES;
    a.tail = (int)(frame_bytes - a.head - a.nvec * VEC_BYTES);
    a.nseg = (a.nvec + THREADS - 1) / THREADS;
    if (a.nseg < 1) a.nseg = 1;
    a.items = a.nseg * ((n_frames + RUN - 1) / RUN);
    return a;
}

// segments of a frame at the alignment that needs the most (a head takes 16 bytes from the vectors at worst, never adding a segment)
inline long long max_segments(long long frame_bytes) {
    const long long nseg = (frame_bytes / VEC_BYTES + THREADS - 1) / THREADS;
    return nseg < 1 ? 1 : nseg;
}

}  // namespace fscan
