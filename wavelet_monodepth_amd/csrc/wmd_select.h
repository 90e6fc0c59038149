// Exact order statistics of float planes by a three-level radix select over 32-bit keys (11 + 11 + 10 bits), and the range of
// a plane's keys -- shared by wmd_eval.hip (np.median for median scaling), wmd_viz.hip (np.percentile, min, max) and
// wmd_dbe.hip (min, max).  Three passes over an item's plane, no scan launches and no host reads in between:
//   sel_pass<0>   histogram of key bits 31..21, and the smallest key
//   sel_pass<1>   every block first finds the bin of level 0 that holds the rank (2048 counts, one scan), then counts bits
//                 20..10 of the keys under that prefix
//   sel_pass<2>   the same one level down (bits 9..0), and the smallest key ABOVE the 22-bit prefix
//   sel_resolve   the key at the rank, and the key at rank + 1: the same key when the last bin holds more than the remaining
//                 rank, else the next occupied bin of level 2, else that smallest key above the prefix
// A block re-derives the prefix from the histograms of the levels above it (8 KB from L2 per level) instead of waiting for a
// one-block launch to do it once.  Histograms are LDS-private per block and flushed once with global atomics (integer adds:
// the counts do not depend on the order).  The callers differ in two things, which are the parameters: the key of a value
// (KEY::of, any map whose unsigned order is the order wanted) and where an item's rank comes from (an argument here).
#pragma once
#include <cstdint>
#include "wmd_internal.h"

namespace wmd {

constexpr int SEL_BINS = 2048;
// uint32 per item, zeroed before level 0: [0] ~min key, [1] ~(smallest key above the prefix), [2..7] the caller's, [8..] histograms
constexpr int SEL_STATE = 8 + 3 * SEL_BINS;
constexpr int SEL_THREADS = 256;              // every function below is written for blocks of this size
constexpr size_t SEL_CHUNK = 4 * SEL_THREADS;   // values a block takes per step of sel_for_each

// f(index, value) over a plane, for grid (blocks, ...): four independent loads in flight per thread; a chunk is 4 x 256
// consecutive values, lane-contiguous in each quarter
template <class F>
__device__ __forceinline__ void sel_for_each(const float* __restrict__ v, size_t plane, F&& f) {
    for (size_t base = (size_t)blockIdx.x * SEL_CHUNK; base < plane; base += (size_t)gridDim.x * SEL_CHUNK) {
        const size_t i = base + threadIdx.x;
        if (base + SEL_CHUNK <= plane) {
            const float a0 = v[i], a1 = v[i + SEL_THREADS], a2 = v[i + 2 * SEL_THREADS], a3 = v[i + 3 * SEL_THREADS];
            f(i, a0);
            f(i + SEL_THREADS, a1);
            f(i + 2 * SEL_THREADS, a2);
            f(i + 3 * SEL_THREADS, a3);
        } else {
            for (int j = 0; j < 4; ++j)
                if (i + j * SEL_THREADS < plane) f(i + j * SEL_THREADS, v[i + j * SEL_THREADS]);
        }
    }
}

// Smallest (and, with MAX, largest) key a thread took, then a wave, then a block.  mn stays 0xFFFFFFFF where nothing was taken.
template <bool MAX>
struct KeyRange {
    unsigned mn = 0xFFFFFFFFu, mx = 0u;
    __device__ __forceinline__ void take(unsigned k) {
        mn = k < mn ? k : mn;
        if (MAX) mx = k > mx ? k : mx;
    }
    // butterfly: every lane ends with its wave's range
    __device__ __forceinline__ void wave() {
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned a = __shfl_xor(mn, o);
            mn = a < mn ? a : mn;
            if (MAX) {
                const unsigned c = __shfl_xor(mx, o);
                mx = c > mx ? c : mx;
            }
        }
    }
    // All 256 threads; sm: 4 uint32 of LDS (8 with MAX).  Every thread ends with the block's range.
    __device__ __forceinline__ void block(unsigned* sm) {
        wave();
        if ((threadIdx.x & 63) == 0) {
            sm[threadIdx.x >> 6] = mn;
            if (MAX) sm[4 + (threadIdx.x >> 6)] = mx;
        }
        __syncthreads();
        mn = min(min(sm[0], sm[1]), min(sm[2], sm[3]));
        if (MAX) mx = max(max(sm[4], sm[5]), max(sm[6], sm[7]));
    }
};

// Publishes ~key into a zeroed word (zero = none yet): one atomic at most, none where it cannot improve what is there
__device__ __forceinline__ void sel_publish_min(unsigned* dst, unsigned key) {
    if (~key > *reinterpret_cast<volatile unsigned*>(dst)) atomicMax(dst, ~key);
}

struct SelFound {
    unsigned bin;     // the bin that holds the rank
    unsigned rem;     // rank inside that bin
    unsigned count;   // keys in that bin
    unsigned next;    // the next occupied bin above it (0xFFFFFFFF: none)
};

// All 256 threads: which of the 2048 bins of `gh` holds 0-based rank `rank`.  sm: 12 uint32 of LDS, reusable on return.
static __device__ SelFound sel_find(const unsigned* __restrict__ gh, unsigned rank, unsigned* sm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned loc[8], sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        loc[j] = gh[tid * 8 + j];
        sum += loc[j];
    }
    unsigned inc = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (tid == 0) {
        sm[4] = SEL_BINS - 1;
        sm[5] = 0;
        sm[6] = 0;
    }
    if (lane == 63) sm[wave] = inc;
    __syncthreads();
    unsigned excl = inc - sum;
    for (int wv = 0; wv < wave; ++wv) excl += sm[wv];
    if (rank >= excl && rank - excl < sum) {      // one thread: the counts are a partition of the ranks
        unsigned cum = 0;
        int j = 0;
        for (; j < 7; ++j) {
            if (cum + loc[j] > rank - excl) break;
            cum += loc[j];
        }
        sm[4] = (unsigned)(tid * 8 + j);
        sm[5] = rank - excl - cum;
        sm[6] = loc[j];
    }
    __syncthreads();
    SelFound f;
    f.bin = sm[4];
    f.rem = sm[5];
    f.count = sm[6];
    unsigned nx = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 7; j >= 0; --j)
        if (loc[j] && (unsigned)(tid * 8 + j) > f.bin) nx = (unsigned)(tid * 8 + j);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = __shfl_xor(nx, o);
        nx = t < nx ? t : nx;
    }
    if (lane == 0) sm[8 + wave] = nx;
    __syncthreads();
    f.next = min(min(sm[8], sm[9]), min(sm[10], sm[11]));
    __syncthreads();
    return f;
}

// One level over the plane `v` of the item whose state is `st`, in a grid of (blocks, ...) x 256 threads.  `rank` is the
// item's 0-based rank (not read at level 0).
template <int LEVEL, class KEY>
__device__ __forceinline__ void sel_pass(const float* __restrict__ v, unsigned* __restrict__ st, size_t plane, unsigned rank) {
    __shared__ unsigned lh[SEL_BINS];
    __shared__ unsigned sm[12];
    for (int i = threadIdx.x; i < SEL_BINS; i += SEL_THREADS) lh[i] = 0;
    unsigned prefix = 0;
    if (LEVEL >= 1) {
        const SelFound f0 = sel_find(st + 8, rank, sm);
        prefix = f0.bin;
        if (LEVEL == 2) {
            const SelFound f1 = sel_find(st + 8 + SEL_BINS, f0.rem, sm);
            prefix = (prefix << 11) | f1.bin;
        }
    }
    __syncthreads();
    constexpr int shift = LEVEL == 0 ? 21 : (LEVEL == 1 ? 10 : 0);
    constexpr unsigned mask = LEVEL == 2 ? 1023u : 2047u;
    KeyRange<false> ext;   // LEVEL 0: smallest key; LEVEL 2: smallest key whose upper 22 bits are above the prefix
    sel_for_each(v, plane, [&](size_t, float value) {
        const unsigned k = KEY::of(value);
        if (LEVEL == 0) {
            atomicAdd(&lh[k >> 21], 1u);
            ext.take(k);
        } else {
            const unsigned hi = LEVEL == 1 ? (k >> 21) : (k >> 10);
            if (hi == prefix) atomicAdd(&lh[(k >> shift) & mask], 1u);
            if (LEVEL == 2 && hi > prefix) ext.take(k);
        }
    });
    __syncthreads();
    unsigned* gh = st + 8 + LEVEL * SEL_BINS;
    for (int i = threadIdx.x; i < SEL_BINS; i += SEL_THREADS)
        if (lh[i]) atomicAdd(&gh[i], lh[i]);
    if (LEVEL != 1) {
        ext.block(sm);
        if (threadIdx.x == 0 && ext.mn != 0xFFFFFFFFu) sel_publish_min(&st[LEVEL == 0 ? 0 : 1], ext.mn);
    }
}

struct SelKeys {
    unsigned at;      // the key at the rank
    unsigned next;    // the key at rank + 1 where it was asked for, else `at` again
};

// All 256 threads, after the three passes.  sm: 12 uint32 of LDS.
__device__ __forceinline__ SelKeys sel_resolve(const unsigned* __restrict__ st, unsigned rank, bool want_next, unsigned* sm) {
    const SelFound f0 = sel_find(st + 8, rank, sm);
    const SelFound f1 = sel_find(st + 8 + SEL_BINS, f0.rem, sm);
    const SelFound f2 = sel_find(st + 8 + 2 * SEL_BINS, f1.rem, sm);
    const unsigned prefix = (f0.bin << 21) | (f1.bin << 10);
    SelKeys s;
    s.at = s.next = prefix | f2.bin;                       // rank + 1: the same key while its bin holds that rank too
    if (want_next && f2.rem + 1 >= f2.count) s.next = f2.next != 0xFFFFFFFFu ? (prefix | f2.next) : ~st[1];
    return s;
}

}  // namespace wmd
