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
//   viz_select_kernel<0,1,2>      the three passes of the radix select of wmd_select.h at rank k; keys = float bits with the
//                                 sign-flip (ascending like the values); level 0 leaves the per-image min
//   viz_colour_kernel<0>          every block resolves the three levels to s[k] and s[k+1].  numpy's float32 lerp,
//                                 matplotlib's double division, the table, and four pixels = three dwords per store.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "wmd_internal.h"
#include "wmd_select.h"
#include "wmd_ws_layouts.h"

// numpy and matplotlib round every operation on its own: no fused multiply-add may be formed from their products.  The
// pragma covers what the front end would fuse; the library is built with the HIP default, under which the back end still
// fuses a product into the sum that follows it, so the one product that feeds a sum here goes through vz_rounded.
#pragma clang fp contract(off)

namespace wmd {

constexpr int VZ_STATE = SEL_STATE;   // uint32 per image: the selection state, with [2] max key
constexpr int VZ_THREADS = SEL_THREADS;

struct VzKey {
    static __device__ __forceinline__ unsigned of(float v) { return order_key(v); }   // ascending like the values
};

// one level of the select (wmd_select.h) over image blockIdx.y; grid (blocks, B)
template <int LEVEL>
__global__ __launch_bounds__(VZ_THREADS) void viz_select_kernel(const float* __restrict__ x, unsigned* __restrict__ state, size_t plane,
                                                               unsigned rank) {
    const int b = blockIdx.y;
    sel_pass<LEVEL, VzKey>(x + (size_t)b * plane, state + (size_t)b * VZ_STATE, plane, rank);
}

// per-image min and max of [B,n] planes, as keys: st[0] = ~min key, st[2] = max key (both zero-initialised)
__global__ __launch_bounds__(VZ_THREADS) void viz_minmax_kernel(const float* __restrict__ x, unsigned* __restrict__ state, size_t plane) {
    const int b = blockIdx.y;
    KeyRange<true> kr;
    sel_for_each(x + (size_t)b * plane, plane, [&](size_t, float value) { kr.take(order_key(value)); });
    __shared__ unsigned sm[8];
    kr.block(sm);
    if (threadIdx.x == 0 && kr.mn != 0xFFFFFFFFu) {      // the block saw at least one value
        unsigned* st = state + (size_t)b * VZ_STATE;
        sel_publish_min(st + 0, kr.mn);
        if (kr.mx > *reinterpret_cast<volatile unsigned*>(st + 2)) atomicMax(st + 2, kr.mx);
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
        const SelKeys k = sel_resolve(st, rank, rank_next != rank, sm);     // s[k] and s[k+1]
        const float lo = order_unkey(~st[0]), hi = vz_lerp(order_unkey(k.at), order_unkey(k.next), g);
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
    float* o = y + (size_t)b * plane;
    sel_for_each(x + (size_t)b * plane, plane, [&](size_t i, float value) { o[i] = __fdiv_rn(__fsub_rn(value, mi), d); });
}

static int vz_blocks(size_t plane, int B, size_t per_block) {
    const size_t want = (plane + per_block - 1) / per_block, cap = std::max<size_t>(8, 2048 / (size_t)B);
    return (int)std::max<size_t>(1, std::min(want, cap));
}

static size_t vz_state_bytes(int B) { return viz_layout(nullptr, B, 0).bytes; }

}  // namespace wmd

using namespace wmd;

extern "C" size_t wmd_viz_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return viz_layout(nullptr, B, (size_t)H * W).bytes;
}

extern "C" int wmd_viz_disparity(const float* disp, int B, int h, int w, int H, int W, double percentile, const unsigned char* lut,
                                 unsigned char* rgb, float* resized, float* range, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    if (!disp || !lut || !rgb || !workspace) return fail(WMD_ERR_BAD_ARG, "wmd_viz_disparity: null pointer (disp, lut, rgb or workspace)");
    if (B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return fail(WMD_ERR_BAD_SHAPE, "wmd_viz_disparity: B=%d h=%d w=%d H=%d W=%d", B, h, w, H, W);
    if (!(percentile >= 0.0 && percentile <= 100.0)) return fail(WMD_ERR_BAD_ARG, "wmd_viz_disparity: percentile %g outside [0, 100]", percentile);
    if ((double)H * W > 2147483647.0) return fail(WMD_ERR_UNSUPPORTED, "wmd_viz_disparity: more than 2^31 pixels per image");
    if (B > 65535) return fail(WMD_ERR_UNSUPPORTED, "wmd_viz_disparity: B=%d above 65535", B);
    const size_t plane = (size_t)H * W;
    if (int st = check_workspace("wmd_viz_disparity", workspace, workspace_bytes, wmd_viz_workspace_bytes(B, H, W), 4, WMD_ERR_BAD_ARG)) return st;
    const VizWs ws = viz_layout(workspace, B, plane);
    hipStream_t s = (hipStream_t)stream;
    // numpy's virtual index of the "linear" method on a float32 array, in float32
    const float qf = (float)percentile / 100.0f;
    const volatile float vi_rounded = (float)(plane - 1) * qf;   // the product, rounded, before the floor is taken off it
    const float vi = vi_rounded;
    const float kf = floorf(vi);
    const float g = vi - kf;
    const unsigned last = (unsigned)(plane - 1);
    const unsigned rank = std::min((unsigned)kf, last), rank_next = std::min(rank + 1, last);
    unsigned* state = ws.state;
    const float* map = disp;
    if (h != H || w != W) {
        float* dst = resized ? resized : ws.resized;
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
    unsigned* state = nullptr;   // stays null with a given range: the colour kernel does not read it then
    if (auto_range) {
        if (!workspace) return fail(WMD_ERR_BAD_ARG, "wmd_viz_colorize: null workspace");
        if (int st = check_workspace("wmd_viz_colorize", workspace, workspace_bytes, vz_state_bytes(B), 4, WMD_ERR_BAD_ARG)) return st;
        state = viz_layout(workspace, B, 0).state;
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
    if (!x || !y || !workspace) return fail(WMD_ERR_BAD_ARG, "wmd_viz_normalize: null pointer (x, y or workspace)");
    if (B <= 0 || n == 0) return fail(WMD_ERR_BAD_SHAPE, "wmd_viz_normalize: B=%d n=%zu", B, n);
    if (B > 65535) return fail(WMD_ERR_UNSUPPORTED, "wmd_viz_normalize: B=%d above 65535", B);
    if (int st = check_workspace("wmd_viz_normalize", workspace, workspace_bytes, vz_state_bytes(B), 4, WMD_ERR_BAD_ARG)) return st;
    hipStream_t s = (hipStream_t)stream;
    unsigned* state = viz_layout(workspace, B, 0).state;
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
