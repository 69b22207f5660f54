// A 64-bit digest of a training state where it lives: one launch over a table of tensors, one small fixed-order finish
// (video_frame_inpainting_amd/run_state.py; the definition is restated in numpy in tests/state_digest_ref.py, which pins it).
//
// Definition, on the raw 32-bit words (an 8-byte element is two words, low word first), all arithmetic in uint64 modulo 2^64:
//   mix(z):   z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
//             return z ^ (z >> 31)                                                     (the splitmix64 output function)
//   entry t with words w[0..n):   E_t = sum_i mix((i << 32) + w[i])
//   digest:   D = 0x243F6A8885A308D3;  for t in table order:  D = mix(D ^ E_t);  D = mix(D + n_t)
// (i << 32) + w is one-to-one in (position, word) below 2^32 words, so a flipped bit, two swapped words or a word that moves to the
// next entry each change one or more terms of a sum of well-mixed values; -0.0 and +0.0 are different words.  The sum is what makes
// the result independent of how the words are cut into segments and of which workgroup takes which: integer addition commutes.  No
// float arithmetic and no atomics: every segment's sum goes to its own workspace slot, and the finish adds the slots of an entry in
// index order and chains the entries in table order.
//
// Table row t (four 64-bit integers, a device copy for the kernels): {address, words n_t, E_t of a host-resident entry, first
// segment}.  An entry on the device is cut into segments of `seg_words` words (a multiple of 4); an entry on the host (address 0,
// its E_t computed by the caller with the same definition) and an empty one have none.
namespace sdig {

constexpr int THREADS = 256;
constexpr int UNROLL = 8;            // 16-byte loads in flight per lane

typedef unsigned int u4v __attribute__((ext_vector_type(4)));
// the addresses come out of the table as integers: said to be global memory, so that the loads are global_load_dwordx4, not flat ones
typedef const __attribute__((address_space(1))) unsigned int* gwords;
typedef const __attribute__((address_space(1))) u4v* gvecs;

__device__ __forceinline__ unsigned long long mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long term(unsigned long long pos, unsigned int w) { return mix((pos << 32) + w); }

// One workgroup per segment, grid-stride over the segments; slot[seg] = the segment's sum.
__global__ __launch_bounds__(THREADS) void segment_sums(const long long* __restrict__ table, int n_entries, long long n_segments,
                                                        long long seg_words, unsigned long long* __restrict__ slot) {
    __shared__ unsigned long long part[THREADS / 64];
    for (long long seg = blockIdx.x; seg < n_segments; seg += gridDim.x) {
        // the last entry whose first segment is <= seg and that has segments at all: first-segment numbers never decrease, entries
        // without segments repeat their successor's, so the LAST row with first <= seg is the owner (uniform over the workgroup)
        int lo = 0, hi = n_entries - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (table[4 * (long long)mid + 3] <= seg) lo = mid; else hi = mid - 1;
        }
        const unsigned long long n = (unsigned long long)table[4 * (long long)lo + 1];
        const unsigned long long first = (unsigned long long)(seg - table[4 * (long long)lo + 3]) * (unsigned long long)seg_words;
        unsigned long long acc = 0;
        if (table[4 * (long long)lo] != 0 && first < n) {           // (a row that does not own the segment contributes nothing)
            const unsigned long long count = n - first < (unsigned long long)seg_words ? n - first : (unsigned long long)seg_words;
            const gwords p = (gwords)(unsigned long long)table[4 * (long long)lo] + first;
            // words in front of the first 16-byte boundary, 16-byte vectors, words behind the last one
            unsigned long long head = ((16 - ((unsigned long long)p & 15)) & 15) >> 2;
            if (head > count) head = count;
            const unsigned long long n_vec = (count - head) >> 2;
            const unsigned long long tail0 = head + 4 * n_vec;
            if (threadIdx.x < head) acc += term(first + threadIdx.x, p[threadIdx.x]);
            if (tail0 + threadIdx.x < count) acc += term(first + tail0 + threadIdx.x, p[tail0 + threadIdx.x]);
            const gvecs pv = (gvecs)(p + head);
            const unsigned long long pos0 = first + head;
            unsigned long long v = threadIdx.x;
            for (; v + (UNROLL - 1) * THREADS < n_vec; v += UNROLL * THREADS) {
                u4v x[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) x[u] = __builtin_nontemporal_load(pv + v + u * THREADS);
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const unsigned long long pos = pos0 + 4 * (v + u * THREADS);
                    acc += term(pos, x[u].x) + term(pos + 1, x[u].y) + term(pos + 2, x[u].z) + term(pos + 3, x[u].w);
                }
            }
            for (; v < n_vec; v += THREADS) {
                const u4v x = __builtin_nontemporal_load(pv + v);
                const unsigned long long pos = pos0 + 4 * v;
                acc += term(pos, x.x) + term(pos + 1, x.y) + term(pos + 2, x.z) + term(pos + 3, x.w);
            }
        }
        // the workgroup's sum: butterflies inside each wave, the four wave sums through LDS
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) slot[seg] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}

// One workgroup: every lane adds the segment sums of its entries in index order (entry_sum[t]), then lane 0 chains the entries in
// table order.
__global__ __launch_bounds__(THREADS) void finish(const long long* __restrict__ table, int n_entries, long long n_segments,
                                                  const unsigned long long* __restrict__ slot, unsigned long long* __restrict__ entry_sum,
                                                  unsigned long long* __restrict__ result) {
    for (int t = threadIdx.x; t < n_entries; t += THREADS) {
        unsigned long long e = (unsigned long long)table[4 * (long long)t + 2];
        if (table[4 * (long long)t] != 0) {
            const long long a = table[4 * (long long)t + 3];
            const long long b = t + 1 < n_entries ? table[4 * (long long)(t + 1) + 3] : n_segments;
            e = 0;
            for (long long s = a; s < b; ++s) e += slot[s];
        }
        entry_sum[t] = e;
    }
    __threadfence();            // the entry sums are read back by lane 0 of this workgroup
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long d = 0x243F6A8885A308D3ULL;
        for (int t = 0; t < n_entries; ++t) {
            d = mix(d ^ entry_sum[t]);
            d = mix(d + (unsigned long long)table[4 * (long long)t + 1]);
        }
        result[0] = d;
    }
}

}  // namespace sdig
