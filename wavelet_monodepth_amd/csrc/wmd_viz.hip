// Colour images of the predictions, for whole batches resident in HBM -- the three places the reference makes them on the host:
//   KITTI/test_simple.py:144-175  F.interpolate -> np.percentile(., 95), .min() -> Normalize -> magma -> * 255 -> uint8
//   NYUv2/utils.py:63-82          colorize: (x - vmin) / (vmax - vmin) over a fixed or the plane's own range -> plasma, bytes
//   KITTI/utils.py:22-28          normalize_image: (x - min) / (max - min)
// The test criterion is the bytes numpy 2.2 and matplotlib 3.10 produce, so every rounding below is theirs (include/wmd.h
// states the rules; tests/viz_ref.py is the same arithmetic in numpy).
//
// wmd_viz_disparity, at most five launches whatever B:
//   upsample_bilinear_fwd_kernel  the existing resample (wmd_resample.hip), skipped when the size does not change; the map is
//                                 written once and read by the four passes below
//   viz_select_kernel<0>          keys = float bits with the sign-flip (ascending like the values); per-image min;
//                                 histogram of key bits 31..21
//   viz_select_kernel<1>          every block first finds the bin of level 0 that holds rank k (2048 counts, one scan), then
//                                 counts bits 20..10 of the keys under that prefix
//   viz_select_kernel<2>          the same one level down (bits 9..0), and the smallest key ABOVE the 22-bit prefix
//   viz_colour_kernel<0>          every block resolves the three levels: s[k] exactly; s[k+1] = s[k] when the last bin holds
//                                 more than the remaining rank, else the next occupied bin of level 2, else that smallest
//                                 key above the prefix.  numpy's float32 lerp, matplotlib's double division, the table, and
//                                 four pixels = three dwords per store.
// No scan kernels and no host reads in between: a block re-derives the prefix from the histograms of the levels above it
// (8 KB from L2 per level) instead of waiting for a one-block launch to do it once.  Histograms are LDS-private per block
// and flushed once with global atomics (integer adds: the counts do not depend on the order).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "wmd_internal.h"

// numpy and matplotlib round every operation on its own: no fused multiply-add may be formed from their products.  The
// pragma covers what the front end would fuse; the library is built with the HIP default, under which the back end still
// fuses a product into the sum that follows it, so the one product that feeds a sum here goes through vz_rounded.
#pragma clang fp contract(off)

namespace wmd {

constexpr int VZ_BINS = 2048;
constexpr int VZ_STATE = 8 + 3 * VZ_BINS;   // uint32 per image: [0] ~min key, [1] ~(smallest key above the prefix), [2] max key, [8..] histograms
constexpr int VZ_THREADS = 256;
constexpr size_t VZ_CHUNK = 4 * VZ_THREADS;   // values a block takes per step of the reducing passes

struct VzFound {
    unsigned bin;     // the bin that holds the rank
    unsigned rem;     // rank inside that bin
    unsigned count;   // keys in that bin
    unsigned next;    // the next occupied bin above it (0xFFFFFFFF: none)
};

// All 256 threads: which of the 2048 bins of `gh` holds 0-based rank `rank`.  sm: 12 uint32 of LDS, reusable on return.
__device__ VzFound vz_find(const unsigned* __restrict__ gh, unsigned rank, unsigned* sm) {
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
        sm[4] = VZ_BINS - 1;
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
    VzFound f;
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

// LEVEL 0: bits 31..21 (+ the min); 1: bits 20..10 under the prefix of level 0; 2: bits 9..0 under the 22-bit prefix (+ the
// smallest key above that prefix).  grid (blocks, B).
template <int LEVEL>
__global__ __launch_bounds__(VZ_THREADS) void viz_select_kernel(const float* __restrict__ x, unsigned* __restrict__ state, size_t plane,
                                                               unsigned rank) {
    const int b = blockIdx.y;
    const float* v = x + (size_t)b * plane;
    unsigned* st = state + (size_t)b * VZ_STATE;
    __shared__ unsigned lh[VZ_BINS];
    __shared__ unsigned sm[12];
    for (int i = threadIdx.x; i < VZ_BINS; i += VZ_THREADS) lh[i] = 0;
    unsigned prefix = 0;
    if (LEVEL >= 1) {
        const VzFound f0 = vz_find(st + 8, rank, sm);
        prefix = f0.bin;
        if (LEVEL == 2) {
            const VzFound f1 = vz_find(st + 8 + VZ_BINS, f0.rem, sm);
            prefix = (prefix << 11) | f1.bin;
        }
    }
    __syncthreads();
    constexpr int shift = LEVEL == 0 ? 21 : (LEVEL == 1 ? 10 : 0);
    constexpr unsigned mask = LEVEL == 2 ? 1023u : 2047u;
    unsigned ext = 0xFFFFFFFFu;   // LEVEL 0: smallest key; LEVEL 2: smallest key whose upper 22 bits are above the prefix
    auto take = [&](float value) {
        const unsigned k = order_key(value);
        if (LEVEL == 0) {
            atomicAdd(&lh[k >> 21], 1u);
            ext = k < ext ? k : ext;
        } else {
            const unsigned hi = LEVEL == 1 ? (k >> 21) : (k >> 10);
            if (hi == prefix) atomicAdd(&lh[(k >> shift) & mask], 1u);
            if (LEVEL == 2 && hi > prefix) ext = k < ext ? k : ext;
        }
    };
    // four independent loads in flight per thread: a chunk is 4 x 256 consecutive values, lane-contiguous in each quarter
    for (size_t base = (size_t)blockIdx.x * VZ_CHUNK; base < plane; base += (size_t)gridDim.x * VZ_CHUNK) {
        const size_t i = base + threadIdx.x;
        if (base + VZ_CHUNK <= plane) {
            const float a0 = v[i], a1 = v[i + VZ_THREADS], a2 = v[i + 2 * VZ_THREADS], a3 = v[i + 3 * VZ_THREADS];
            take(a0);
            take(a1);
            take(a2);
            take(a3);
        } else {
            for (int j = 0; j < 4; ++j)
                if (i + j * VZ_THREADS < plane) take(v[i + j * VZ_THREADS]);
        }
    }
    __syncthreads();
    unsigned* gh = st + 8 + LEVEL * VZ_BINS;
    for (int i = threadIdx.x; i < VZ_BINS; i += VZ_THREADS)
        if (lh[i]) atomicAdd(&gh[i], lh[i]);
    if (LEVEL != 1) {
        // one atomic per block at most, stored inverted (zero = none yet); a block that cannot improve what it reads sends none
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned t = __shfl_xor(ext, o);
            ext = t < ext ? t : ext;
        }
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = ext;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned m = min(min(sm[0], sm[1]), min(sm[2], sm[3]));
            unsigned* dst = &st[LEVEL == 0 ? 0 : 1];
            if (m != 0xFFFFFFFFu && ~m > *reinterpret_cast<volatile unsigned*>(dst)) atomicMax(dst, ~m);
        }
    }
}

// per-image min and max of [B,n] planes, as keys: st[0] = ~min key, st[2] = max key (both zero-initialised)
__global__ __launch_bounds__(VZ_THREADS) void viz_minmax_kernel(const float* __restrict__ x, unsigned* __restrict__ state, size_t plane) {
    const int b = blockIdx.y;
    const float* v = x + (size_t)b * plane;
    unsigned mn = 0xFFFFFFFFu, mx = 0u;
    auto take = [&](float value) {
        const unsigned k = order_key(value);
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
    };
    for (size_t base = (size_t)blockIdx.x * VZ_CHUNK; base < plane; base += (size_t)gridDim.x * VZ_CHUNK) {
        const size_t i = base + threadIdx.x;
        if (base + VZ_CHUNK <= plane) {
            const float a0 = v[i], a1 = v[i + VZ_THREADS], a2 = v[i + 2 * VZ_THREADS], a3 = v[i + 3 * VZ_THREADS];
            take(a0);
            take(a1);
            take(a2);
            take(a3);
        } else {
            for (int j = 0; j < 4; ++j)
                if (i + j * VZ_THREADS < plane) take(v[i + j * VZ_THREADS]);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = __shfl_xor(mn, o), c = __shfl_xor(mx, o);
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
    __shared__ unsigned sm[8];
    if ((threadIdx.x & 63) == 0) {
        sm[threadIdx.x >> 6] = mn;
        sm[4 + (threadIdx.x >> 6)] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = min(min(sm[0], sm[1]), min(sm[2], sm[3]));
        mx = max(max(sm[4], sm[5]), max(sm[6], sm[7]));
        unsigned* st = state + (size_t)b * VZ_STATE;
        if (mn != 0xFFFFFFFFu) {      // the block saw at least one value
            if (~mn > *reinterpret_cast<volatile unsigned*>(st + 0)) atomicMax(st + 0, ~mn);
            if (mx > *reinterpret_cast<volatile unsigned*>(st + 2)) atomicMax(st + 2, mx);
        }
    }
}

// a value the optimiser has to take as it is: the product behind it is rounded before anything is added to it
__device__ __forceinline__ float vz_rounded(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// numpy's _lerp on float32: from the left below g = 0.5, from the right from there on, every operation rounded
__device__ __forceinline__ float vz_lerp(float a, float b, float g) {
    const float d = vz_rounded(b - a);
    return g < 0.5f ? a + vz_rounded(d * g) : b - vz_rounded(d * vz_rounded(1.f - g));
}

// matplotlib's Colormap.__call__ on a float32 array: * N, under -> first row, over (and exactly N) -> last row, truncation
__device__ __forceinline__ unsigned vz_lookup(float t, const unsigned* lut) {
    const float xa = __fmul_rn(t, 256.f);
    if (xa != xa) return 0u;                    // the bad colour (0, 0, 0)
    const int idx = xa < 0.f ? 0 : (xa >= 256.f ? 255 : (int)xa);
    return lut[idx];
}

struct VzNorm {
    float lo, den_f;    // MODE 1 / 2: float32 arithmetic
    double lo_d, den_d; // MODE 0: matplotlib's Normalize, float64 scalars on a float32 array
    bool flat;          // every pixel gets the first row
};

template <int MODE>
__device__ __forceinline__ unsigned vz_colour(float x, const VzNorm& nm, const unsigned* lut) {
    if (nm.flat) return (MODE == 1 && x != x) ? 0u : lut[0];   // colorize multiplies by zero there: NaN stays the bad colour
    float t;
    if (MODE == 0) {
        t = (float)((double)x - nm.lo_d);       // resdat -= vmin: in double, rounded into the float32 array
        t = (float)((double)t / nm.den_d);      // resdat /= (vmax - vmin)
    } else {
        t = __fdiv_rn(__fsub_rn(x, nm.lo), nm.den_f);
    }
    return vz_lookup(t, lut);
}

// MODE 0: wmd_viz_disparity's last pass (range from the selection state); MODE 1: wmd_viz_colorize (fixed range, or the
// plane's own from viz_minmax_kernel).  out: [B,n,3], or [B,3,n] when chw.  packed: four pixels per thread and dword stores
// (the host checked the alignment); the pixels in front of the first aligned group, behind the last one, or all of them when
// !packed, take byte stores.  grid (blocks, B).
template <int MODE>
__global__ __launch_bounds__(VZ_THREADS) void viz_colour_kernel(const float* __restrict__ x, const unsigned* __restrict__ state,
                                                               const unsigned char* __restrict__ lut768, unsigned char* __restrict__ out,
                                                               float* __restrict__ range, size_t plane, unsigned rank, unsigned rank_next,
                                                               float g, int auto_range, float vmin, float den, int chw, int packed) {
    const int b = blockIdx.y;
    __shared__ unsigned lut[256];
    __shared__ unsigned sm[12];
    lut[threadIdx.x] = (unsigned)lut768[threadIdx.x * 3] | ((unsigned)lut768[threadIdx.x * 3 + 1] << 8) | ((unsigned)lut768[threadIdx.x * 3 + 2] << 16);
    VzNorm nm;
    nm.lo = vmin;
    nm.den_f = den;
    nm.lo_d = nm.den_d = 0.0;
    nm.flat = false;
    if (MODE == 0) {
        const unsigned* st = state + (size_t)b * VZ_STATE;
        const VzFound f0 = vz_find(st + 8, rank, sm);
        const VzFound f1 = vz_find(st + 8 + VZ_BINS, f0.rem, sm);
        const VzFound f2 = vz_find(st + 8 + 2 * VZ_BINS, f1.rem, sm);
        const unsigned prefix = (f0.bin << 21) | (f1.bin << 10);
        const unsigned ka = prefix | f2.bin;
        unsigned kb = ka;                                        // s[k+1]: the same value while its bin holds rank + 1 too
        if (rank_next != rank && f2.rem + 1 >= f2.count) kb = f2.next != 0xFFFFFFFFu ? (prefix | f2.next) : ~st[1];
        const float lo = order_unkey(~st[0]), hi = vz_lerp(order_unkey(ka), order_unkey(kb), g);
        nm.lo_d = (double)lo;
        nm.den_d = (double)hi - (double)lo;
        nm.flat = lo == hi;
        if (range && blockIdx.x == 0 && threadIdx.x == 0) {
            range[b * 2 + 0] = lo;
            range[b * 2 + 1] = hi;
        }
    } else if (auto_range) {
        const unsigned* st = state + (size_t)b * VZ_STATE;
        const float lo = order_unkey(~st[0]), hi = order_unkey(st[2]);
        nm.lo = lo;
        nm.den_f = __fsub_rn(hi, lo);
        nm.flat = nm.den_f == 0.f;
    } else {
        nm.flat = den == 0.f;
    }
    __syncthreads();
    const float* v = x + (size_t)b * plane;
    unsigned char* o = out + (size_t)b * plane * 3;
    const size_t gtid = (size_t)blockIdx.x * VZ_THREADS + threadIdx.x, gstride = (size_t)gridDim.x * VZ_THREADS;
    // interleaved: byte (b plane + p) 3 is dword-aligned for p = lead (mod 4); planar: the host passes packed only when n % 4 == 0
    size_t lead = packed ? (chw ? 0 : (((size_t)b * plane * 3) & 3)) : plane;
    lead = lead < plane ? lead : plane;
    const size_t groups = (plane - lead) / 4, tail0 = lead + groups * 4;
    for (size_t gi = gtid; gi < groups; gi += gstride) {
        const size_t p = lead + gi * 4;
        const unsigned c0 = vz_colour<MODE>(v[p], nm, lut), c1 = vz_colour<MODE>(v[p + 1], nm, lut);
        const unsigned c2 = vz_colour<MODE>(v[p + 2], nm, lut), c3 = vz_colour<MODE>(v[p + 3], nm, lut);
        if (chw) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int s = 8 * c;
                *reinterpret_cast<unsigned*>(o + (size_t)c * plane + p) =
                    ((c0 >> s) & 255u) | (((c1 >> s) & 255u) << 8) | (((c2 >> s) & 255u) << 16) | (((c3 >> s) & 255u) << 24);
            }
        } else {
            unsigned* q = reinterpret_cast<unsigned*>(o + p * 3);
            q[0] = c0 | (c1 << 24);
            q[1] = (c1 >> 8) | (c2 << 16);
            q[2] = (c2 >> 16) | (c3 << 8);
        }
    }
    const size_t loose = lead + (plane - tail0);
    for (size_t s = gtid; s < loose; s += gstride) {
        const size_t p = s < lead ? s : tail0 + (s - lead);
        const unsigned c = vz_colour<MODE>(v[p], nm, lut);
        if (chw) {
            o[p] = (unsigned char)(c & 255u);
            o[plane + p] = (unsigned char)((c >> 8) & 255u);
            o[2 * plane + p] = (unsigned char)((c >> 16) & 255u);
        } else {
            o[p * 3] = (unsigned char)(c & 255u);
            o[p * 3 + 1] = (unsigned char)((c >> 8) & 255u);
            o[p * 3 + 2] = (unsigned char)((c >> 16) & 255u);
        }
    }
}

// y = (x - min) / d, d = max - min taken in double and rounded to float32, 1e5 for a constant plane
__global__ __launch_bounds__(VZ_THREADS) void viz_normalize_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                  const unsigned* __restrict__ state, size_t plane) {
    const int b = blockIdx.y;
    const unsigned* st = state + (size_t)b * VZ_STATE;
    const float mi = order_unkey(~st[0]), ma = order_unkey(st[2]);
    const float d = ma != mi ? (float)((double)ma - (double)mi) : 1e5f;
    const float* v = x + (size_t)b * plane;
    float* o = y + (size_t)b * plane;
    for (size_t base = (size_t)blockIdx.x * VZ_CHUNK; base < plane; base += (size_t)gridDim.x * VZ_CHUNK) {
        const size_t i = base + threadIdx.x;
        if (base + VZ_CHUNK <= plane) {
            const float a0 = v[i], a1 = v[i + VZ_THREADS], a2 = v[i + 2 * VZ_THREADS], a3 = v[i + 3 * VZ_THREADS];
            o[i] = __fdiv_rn(__fsub_rn(a0, mi), d);
            o[i + VZ_THREADS] = __fdiv_rn(__fsub_rn(a1, mi), d);
            o[i + 2 * VZ_THREADS] = __fdiv_rn(__fsub_rn(a2, mi), d);
            o[i + 3 * VZ_THREADS] = __fdiv_rn(__fsub_rn(a3, mi), d);
        } else {
            for (int j = 0; j < 4; ++j)
                if (i + j * VZ_THREADS < plane) o[i + j * VZ_THREADS] = __fdiv_rn(__fsub_rn(v[i + j * VZ_THREADS], mi), d);
        }
    }
}

static int vz_blocks(size_t plane, int B, size_t per_block) {
    const size_t want = (plane + per_block - 1) / per_block, cap = std::max<size_t>(8, 2048 / (size_t)B);
    return (int)std::max<size_t>(1, std::min(want, cap));
}

static size_t vz_state_bytes(int B) { return (size_t)B * VZ_STATE * sizeof(unsigned); }

}  // namespace wmd

using namespace wmd;

extern "C" size_t wmd_viz_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    // [B] selection states (min, the key above the prefix, max, three histograms), then one resized plane per image
    return vz_state_bytes(B) + (size_t)B * H * W * sizeof(float);
}

extern "C" int wmd_viz_disparity(const float* disp, int B, int h, int w, int H, int W, double percentile, const unsigned char* lut,
                                 unsigned char* rgb, float* resized, float* range, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    if (!disp || !lut || !rgb || !workspace) return fail(WMD_ERR_BAD_ARG, "wmd_viz_disparity: null pointer");
    if (B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return fail(WMD_ERR_BAD_SHAPE, "wmd_viz_disparity: B=%d h=%d w=%d H=%d W=%d", B, h, w, H, W);
    if (!(percentile >= 0.0 && percentile <= 100.0)) return fail(WMD_ERR_BAD_ARG, "wmd_viz_disparity: percentile %g outside [0, 100]", percentile);
    if ((double)H * W > 2147483647.0) return fail(WMD_ERR_UNSUPPORTED, "wmd_viz_disparity: more than 2^31 pixels per image");
    if (B > 65535) return fail(WMD_ERR_UNSUPPORTED, "wmd_viz_disparity: B=%d above 65535", B);
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return fail(WMD_ERR_BAD_ARG, "wmd_viz_disparity: workspace not 4-byte aligned");
    const size_t need = wmd_viz_workspace_bytes(B, H, W);
    if (workspace_bytes < need) return fail(WMD_ERR_WORKSPACE, "wmd_viz_disparity: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const size_t plane = (size_t)H * W;
    // numpy's virtual index of the "linear" method on a float32 array, in float32
    const float qf = (float)percentile / 100.0f;
    const volatile float vi_rounded = (float)(plane - 1) * qf;   // the product, rounded, before the floor is taken off it
    const float vi = vi_rounded;
    const float kf = floorf(vi);
    const float g = vi - kf;
    const unsigned last = (unsigned)(plane - 1);
    const unsigned rank = std::min((unsigned)kf, last), rank_next = std::min(rank + 1, last);
    unsigned* state = reinterpret_cast<unsigned*>(workspace);
    const float* map = disp;
    if (h != H || w != W) {
        float* dst = resized ? resized : reinterpret_cast<float*>(state + (size_t)B * VZ_STATE);
        const int st = wmd_upsample_bilinear_fwd(disp, dst, nullptr, B, h, w, H, W, 0, 0.f, 0.f, stream);
        if (st) return st;
        map = dst;
    } else if (resized) {
        if (hipMemcpyAsync(resized, disp, sizeof(float) * B * plane, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(WMD_ERR_HIP, "wmd_viz_disparity: hipMemcpyAsync failed");
    }
    if (hipMemsetAsync(state, 0, vz_state_bytes(B), s) != hipSuccess) return fail(WMD_ERR_HIP, "wmd_viz_disparity: hipMemsetAsync failed");
    const int nblk = vz_blocks(plane, B, 2048);
    const double bytes = 4.0 * B * plane;
    {
        ProfScope prof("viz_select_kernel<0>", 0.0, bytes, s);
        hipLaunchKernelGGL(viz_select_kernel<0>, dim3(nblk, B), dim3(VZ_THREADS), 0, s, map, state, plane, rank);
    }
    {
        ProfScope prof("viz_select_kernel<1>", 0.0, bytes, s);
        hipLaunchKernelGGL(viz_select_kernel<1>, dim3(nblk, B), dim3(VZ_THREADS), 0, s, map, state, plane, rank);
    }
    {
        ProfScope prof("viz_select_kernel<2>", 0.0, bytes, s);
        hipLaunchKernelGGL(viz_select_kernel<2>, dim3(nblk, B), dim3(VZ_THREADS), 0, s, map, state, plane, rank);
    }
    int st = check_launch("viz_select_kernel");
    if (st) return st;
    const int packed = (reinterpret_cast<uintptr_t>(rgb) & 3) == 0;
    ProfScope prof("viz_colour_kernel<disparity>", 0.0, 7.0 * B * plane, s);
    hipLaunchKernelGGL(viz_colour_kernel<0>, dim3(vz_blocks(plane, B, 4096), B), dim3(VZ_THREADS), 0, s, map, state, lut, rgb, range, plane,
                       rank, rank_next, g, 0, 0.f, 0.f, 0, packed);
    return check_launch("viz_colour_kernel");
}

extern "C" int wmd_viz_colorize(const float* x, int B, size_t n, int auto_range, float vmin, float den, const unsigned char* lut,
                                unsigned char* out, int channels_first, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !lut || !out) return fail(WMD_ERR_BAD_ARG, "wmd_viz_colorize: null pointer");
    if (B <= 0 || n == 0) return fail(WMD_ERR_BAD_SHAPE, "wmd_viz_colorize: B=%d n=%zu", B, n);
    if (B > 65535) return fail(WMD_ERR_UNSUPPORTED, "wmd_viz_colorize: B=%d above 65535", B);
    hipStream_t s = (hipStream_t)stream;
    unsigned* state = reinterpret_cast<unsigned*>(workspace);
    if (auto_range) {
        if (!workspace) return fail(WMD_ERR_BAD_ARG, "wmd_viz_colorize: null workspace");
        if (reinterpret_cast<uintptr_t>(workspace) & 3) return fail(WMD_ERR_BAD_ARG, "wmd_viz_colorize: workspace not 4-byte aligned");
        if (workspace_bytes < vz_state_bytes(B))
            return fail(WMD_ERR_WORKSPACE, "wmd_viz_colorize: workspace %zu < %zu bytes", workspace_bytes, vz_state_bytes(B));
        if (hipMemsetAsync(state, 0, vz_state_bytes(B), s) != hipSuccess) return fail(WMD_ERR_HIP, "wmd_viz_colorize: hipMemsetAsync failed");
        ProfScope prof("viz_minmax_kernel", 0.0, 4.0 * B * n, s);
        hipLaunchKernelGGL(viz_minmax_kernel, dim3(vz_blocks(n, B, 4096), B), dim3(VZ_THREADS), 0, s, x, state, n);
        const int st = check_launch("viz_minmax_kernel");
        if (st) return st;
    } else if (!(den == den) || !(vmin == vmin)) {
        return fail(WMD_ERR_BAD_ARG, "wmd_viz_colorize: the range is not a number");
    }
    const int aligned = (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    const int packed = aligned && (!channels_first || n % 4 == 0);
    ProfScope prof("viz_colour_kernel<colorize>", 0.0, 7.0 * B * n, s);
    hipLaunchKernelGGL(viz_colour_kernel<1>, dim3(vz_blocks(n, B, 4096), B), dim3(VZ_THREADS), 0, s, x, state, lut, out, (float*)nullptr, n, 0u, 0u,
                       0.f, auto_range ? 1 : 0, vmin, den, channels_first ? 1 : 0, packed);
    return check_launch("viz_colour_kernel");
}

extern "C" int wmd_viz_normalize(const float* x, float* y, int B, size_t n, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !y || !workspace) return fail(WMD_ERR_BAD_ARG, "wmd_viz_normalize: null pointer");
    if (B <= 0 || n == 0) return fail(WMD_ERR_BAD_SHAPE, "wmd_viz_normalize: B=%d n=%zu", B, n);
    if (B > 65535) return fail(WMD_ERR_UNSUPPORTED, "wmd_viz_normalize: B=%d above 65535", B);
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return fail(WMD_ERR_BAD_ARG, "wmd_viz_normalize: workspace not 4-byte aligned");
    if (workspace_bytes < vz_state_bytes(B))
        return fail(WMD_ERR_WORKSPACE, "wmd_viz_normalize: workspace %zu < %zu bytes", workspace_bytes, vz_state_bytes(B));
    hipStream_t s = (hipStream_t)stream;
    unsigned* state = reinterpret_cast<unsigned*>(workspace);
    if (hipMemsetAsync(state, 0, vz_state_bytes(B), s) != hipSuccess) return fail(WMD_ERR_HIP, "wmd_viz_normalize: hipMemsetAsync failed");
    const int nblk = vz_blocks(n, B, 4096);
    {
        ProfScope prof("viz_minmax_kernel", 0.0, 4.0 * B * n, s);
        hipLaunchKernelGGL(viz_minmax_kernel, dim3(nblk, B), dim3(VZ_THREADS), 0, s, x, state, n);
    }
    ProfScope prof("viz_normalize_kernel", 0.0, 8.0 * B * n, s);
    hipLaunchKernelGGL(viz_normalize_kernel, dim3(nblk, B), dim3(VZ_THREADS), 0, s, x, y, state, n);
    return check_launch("viz_normalize_kernel");
}
