// The frame scan's four integers per BLOCK of every frame (included by sepconv_capi.hip after frame_scan.hip.inc, whose load16 and
// add_word it shares): what restore.py tells partly damaged frames by.  The definition is the one include/tai_sepconv.h writes down for
// tai_block_scan and tests/block_scan_ref.py restates in numpy.  Frames are uint8 [h][w][c]; block (by, bx) of a frame is its pixels
// [by bs, min(h, by bs + bs)) x [bx bs, min(w, bx bs + bs)), all channels; for block (by, bx) of frame i, over the bytes of that block,
//   s1 = sum v;  s2 = sum v * v;  sad = sum |v_i - v_{i-1}|;  ndiff = #{ |v_i - v_{i-1}| > tol }   (sad = ndiff = 0 for i = 0).
// Sums of non-negative integers: one correct bit pattern whatever the order.  Row i reads frames i - 1 and i and nothing else.
//
// Lanes to blocks.  A pixel row of a block is bs c bytes, a multiple of 8 (bs >= 8).  A row of the frame is cut, from its FIRST BYTE
// (not from an aligned address), into segments of NB = floor(1024 / (bs c)) whole blocks, and a segment into 16-byte chunks, one per lane
// of a wave (64 chunks = 1024 bytes, which NB blocks never exceed).  A chunk starts a multiple of 16 behind a multiple of bs c, i.e. at a
// multiple of 8 of the row, so it never holds bytes of three blocks: its low 8 bytes lie in one block and its high 8 bytes in one block
// (the same one, or the next when bs c is 8, 24, 48 or 96).  A lane therefore keeps two sets of sums, `lo` and `hi`, and never looks at a
// byte's block: the 8-byte unit u = 2 chunk + half of a segment belongs to block u / (bs c / 8) of it.  Bytes behind the row's or the
// segment's end are read as 0 in both frames (single byte loads, and only in the chunk that holds the end): they add nothing to any sum.
//
// Work split.  A work item is (run of RUN frames, block row, segment).  The four waves of the workgroup take rows wave, wave + 4, ... of
// the block row (bs / 4 passes); in a pass a lane issues the loads of its chunk in the RUN frames and in the frame before the run up front
// (RUN + 1 loads of 16 bytes in flight), then walks the run with the previous frame's chunk in registers, like the frame scan: every
// byte of the video is read 1 + 1 / RUN times.  A row's address has the same low four bits in all lanes of a wave, so load16's choice
// of 16-byte, 4-byte or single loads is uniform.  After the passes the lane's 2 x 4 sums of each frame go through LDS as 32-bit words
// ([statistic][wave][unit], double buffered: one barrier per frame) and each (block, statistic) of the segment is added by one thread
// from its bs c / 8 units of the four waves.  A block is complete inside one work item, so there is no workspace, no second launch and
// no atomics.  The grid is capped at GRID_CAP workgroups; past it a workgroup strides.
//
// Accumulators: a block holds at most 32 * 32 * 4 = 4096 bytes and 4096 * 255 * 255 < 2^32, so the 32-bit sums of a lane (at most
// 16 bytes x 8 passes) and of a block cannot overflow, not even s2 at all-255 input; the output is int64.

namespace bscan {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int RUN = 8;                                 // frames per work item
constexpr int VEC_BYTES = 16;
constexpr int UNIT_BYTES = 8;                          // what a lane's `lo` and `hi` sums each cover
constexpr int SEG_BYTES = 64 * VEC_BYTES;              // bytes of a row a wave covers: NB = SEG_BYTES / (bs c) whole blocks
constexpr int UNITS = SEG_BYTES / UNIT_BYTES;          // 128
constexpr long long GRID_CAP = 1LL << 14;
constexpr int STATS = 4;                               // s1, s2, sad, ndiff
constexpr int MAX_BLOCK_BYTES = 32 * 32 * 4;
constexpr long long MAX_TOTAL_BYTES = 1LL << 40;       // n_frames * h * w * c: every byte offset and output index stays below 2^47

static_assert((unsigned long long)MAX_BLOCK_BYTES * 255 * 255 < (1ULL << 32), "32-bit lane and block accumulators hold a whole block at all-255 input");
static_assert(RUN == fscan::RUN, "the block scan reads every byte as often as the frame scan");

struct Args {
    const unsigned char* frames;
    long long* stats;              // [n_frames][Bh][Bw][STATS]
    long long n_frames, items;     // items = ceil(n_frames / RUN) * Bh * nseg
    int h, w, c, bs, tol;
    int row_bytes;                 // w c
    int Bh, Bw;
    int nb;                        // whole blocks of a segment
    int nseg;                      // ceil(Bw / nb)
    int upb;                       // 8-byte units of a block's pixel row: bs c / 8
};

// the chunk at q, of which only the first `valid` (0..16) bytes belong to this lane's segment and row: the others read as 0
__device__ __forceinline__ uint4 load_chunk(const unsigned char* q, int valid) {
    if (valid >= VEC_BYTES) return fscan::load16(q);
    unsigned d[4] = {0u, 0u, 0u, 0u};
    const volatile unsigned char* b = q;
#pragma unroll
    for (int k = 0; k < VEC_BYTES - 1; ++k)
        if (k < valid) d[k >> 2] |= (unsigned)b[k] << (8 * (k & 3));
    return make_uint4(d[0], d[1], d[2], d[3]);
}

template <bool TOL0>
__global__ __launch_bounds__(THREADS)
void walk(const Args a) {
    __shared__ unsigned unit_sums[2][STATS][WAVES][UNITS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long long n = a.n_frames;
    const long long frame_bytes = (long long)a.h * a.row_bytes;
    const unsigned tol2 = 2u * (unsigned)a.tol;
    const fscan::us2 tolv = {(unsigned short)a.tol, (unsigned short)a.tol};
    const long long per_run = (long long)a.Bh * a.nseg;

    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long r = item / per_run;
        const int rest = (int)(item - r * per_run);
        const int by = rest / a.nseg, s = rest - by * a.nseg;
        const long long f0 = r * RUN;                                        // the run's first frame
        const int nf = (int)(n - f0 < RUN ? n - f0 : RUN);                   // its frames, 1..RUN
        const int b0 = s * a.nb;                                             // the segment's first block column
        const int nblk = a.Bw - b0 < a.nb ? a.Bw - b0 : a.nb;                // its blocks, 1..nb
        const int seg_start = b0 * a.upb * UNIT_BYTES;                       // in bytes of the row
        const int seg_full = seg_start + nblk * a.upb * UNIT_BYTES;
        const int seg_end = seg_full < a.row_bytes ? seg_full : a.row_bytes; // the last block of a row may be ragged
        const int x0 = seg_start + lane * VEC_BYTES;
        const int valid = seg_end - x0 < 0 ? 0 : (seg_end - x0 > VEC_BYTES ? VEC_BYTES : seg_end - x0);
        const int y_end = (by + 1) * a.bs < a.h ? (by + 1) * a.bs : a.h;

        unsigned lo[RUN][STATS], hi[RUN][STATS];
#pragma unroll
        for (int j = 0; j < RUN; ++j)
#pragma unroll
            for (int q = 0; q < STATS; ++q) lo[j][q] = hi[j][q] = 0u;

        for (int y = by * a.bs + wave; y < y_end; y += WAVES) {
            // slot j holds frame f0 - 1 + j: slot 0 is the frame before the run (absent for the first run, never used then)
            uint4 v[RUN + 1];
#pragma unroll
            for (int j = 0; j <= RUN; ++j) {
                const long long f = f0 - 1 + j;
                v[j] = make_uint4(0u, 0u, 0u, 0u);
                if (f >= 0 && j <= nf && valid > 0) v[j] = load_chunk(a.frames + f * frame_bytes + (long long)y * a.row_bytes + x0, valid);
            }
#pragma unroll
            for (int j = 1; j <= RUN; ++j) {
                if (j <= nf) {
                    fscan::add_word<TOL0>(v[j].x, v[j - 1].x, tol2, tolv, lo[j - 1][0], lo[j - 1][1], lo[j - 1][2], lo[j - 1][3]);
                    fscan::add_word<TOL0>(v[j].y, v[j - 1].y, tol2, tolv, lo[j - 1][0], lo[j - 1][1], lo[j - 1][2], lo[j - 1][3]);
                    fscan::add_word<TOL0>(v[j].z, v[j - 1].z, tol2, tolv, hi[j - 1][0], hi[j - 1][1], hi[j - 1][2], hi[j - 1][3]);
                    fscan::add_word<TOL0>(v[j].w, v[j - 1].w, tol2, tolv, hi[j - 1][0], hi[j - 1][1], hi[j - 1][2], hi[j - 1][3]);
                }
            }
        }
        if (f0 == 0) { lo[0][2] = lo[0][3] = hi[0][2] = hi[0][3] = 0u; }    // frame 0 has no frame before it

#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            if (j < nf) {                                                    // uniform: nf is the work item's
                unsigned (*buf)[WAVES][UNITS] = unit_sums[j & 1];
#pragma unroll
                for (int q = 0; q < STATS; ++q) {
                    buf[q][wave][2 * lane] = lo[j][q];
                    buf[q][wave][2 * lane + 1] = hi[j][q];
                }
                // one barrier per frame: a thread that writes buffer j & 1 again (frame j + 2) has passed the barrier of frame j + 1, which
                // every thread reaches only after its reads of frame j
                __syncthreads();
                long long* out = a.stats + (((f0 + j) * a.Bh + by) * a.Bw + b0) * STATS;
                for (int o = t; o < nblk * STATS; o += THREADS) {
                    const int b = o >> 2, q = o & 3;
                    unsigned acc = 0u;
                    for (int u = b * a.upb; u < (b + 1) * a.upb; ++u)
#pragma unroll
                        for (int w = 0; w < WAVES; ++w) acc += buf[q][w][u];
                    out[o] = (long long)acc;
                }
            }
        }
        __syncthreads();          // the last two frames' sums are read before the next item writes them
    }
}

// what tai_block_scan and its workspace query refuse for the sizes; null: they are taken
inline const char* refusal(long long n_frames, int h, int w, int c, int bs) {
    if (n_frames < 1) return "block_scan: n_frames must be >= 1";
    if (h < 1 || w < 1) return "block_scan: h and w must be >= 1";
    if (c < 1 || c > 4) return "block_scan: c must be in 1..4";
    if (bs != 8 && bs != 16 && bs != 32) return "block_scan: bs must be 8, 16 or 32";
    if ((long long)h * w * c >= (1LL << 31)) return "block_scan: h x w x c must be below 2^31";
    if (n_frames > MAX_TOTAL_BYTES / ((long long)h * w * c)) return "block_scan: n_frames x h x w x c must not exceed 2^40";
    return nullptr;
}

// bytes of workspace: none -- every block is complete inside one work item
inline long long workspace_bytes(long long, int, int, int, int) { return 0; }

// everything tai_block_scan refuses, before any runtime call; null: the launch goes ahead
inline const char* call_refusal(const unsigned char* frames, long long n_frames, int h, int w, int c, int bs, int tol, const long long* stats,
                                const void* workspace) {
    if (!frames) return "block_scan: frames is a null pointer";
    if (!stats) return "block_scan: stats is a null pointer";
    if (const char* why = refusal(n_frames, h, w, c, bs)) return why;
    if (tol < 0 || tol > 254) return "block_scan: tol must be in 0..254";
    if (reinterpret_cast<uintptr_t>(stats) % 8 || (workspace_bytes(n_frames, h, w, c, bs) > 0 && reinterpret_cast<uintptr_t>(workspace) % 8))
        return "block_scan: stats and a non-empty workspace must be 8-byte aligned";
    return nullptr;
}

// the cut of the frames (taken sizes only)
inline Args plan(long long n_frames, int h, int w, int c, int bs) {
    Args a = {};
    a.n_frames = n_frames;
    a.h = h; a.w = w; a.c = c; a.bs = bs;
    a.row_bytes = w * c;
    a.Bh = (h + bs - 1) / bs;
    a.Bw = (w + bs - 1) / bs;
    a.upb = bs * c / UNIT_BYTES;
    a.nb = UNITS / a.upb;
    a.nseg = (a.Bw + a.nb - 1) / a.nb;
    a.items = ((n_frames + RUN - 1) / RUN) * a.Bh * a.nseg;
    return a;
}

}  // namespace bscan
