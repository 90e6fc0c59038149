// KITTI training inputs (KITTI/datasets/mono_dataset.py:118-145, MonoDataset.preprocess): N decoded uint8 frames [N,H0,W0,3] ->
// per scale the uint8 level, ("color", f, s) and ("color_aug", f, s) as float32 CHW, bit for bit what the reference's chain over
// Pillow gives: flip, 8-bit Lanczos resize (each level from the previous one), ToTensor, torchvision 0.8.2's ColorJitter on
// PIL images.  Everything is integer or float32 / float64 arithmetic with every operation rounded on its own, hence the
// file-wide `fp contract(off)` below: Pillow's x86 build has no fused multiply-add, and hipcc contracts a * b + c by default
// (also through __fmul_rn / __fadd_rn, which are plain operators in HIP).
//
//   wmd_resample.h          the Lanczos tables (host; they depend on (in, out) only), the fixed-point pass and its clamped windows
//   resize_level_kernel     one launch per level (the levels are a dependent chain).  A block owns 64 x th output pixels of one
//                           image: horizontal pass over the tile's clipped row footprint into a uint8 LDS intermediate (the
//                           flip is a mirrored gather here, source column W - 1 - x: the fixed-point tables are not mirror
//                           symmetric, so flipping the result would differ), vertical pass from LDS, uint8 level to HBM.  With
//                           jitter on it applies the ops ordered before contrast to its output pixels and adds their grey
//                           values to a 64-bit counter per (level, image): an integer sum, the same bits in any order.
//   finish_kernel           one launch over all levels: uint8 -> color = u8 / 255 (a float32 division), the whole jitter chain with
//                           the mean m = (2 sum + n) / (2 n) -> color_aug; planar stores, one plane per instruction.
//   jitter_sum_kernel       wmd_color_jitter's reduction (no resize launch to ride on), then finish_kernel writes uint8.
//
// Source pixels are read with byte loads: a native row is 3 W0 bytes (3726 at W0 = 1242) and starts on no dword boundary, and
// a byte load can read neither before a row's first byte nor past the last byte of the last image.  Every index that comes
// out of a device-side table or parameter array is clamped to the tensor it addresses.
#include <algorithm>
#include "wmd_internal.h"
#include "wmd_resample.h"
#include "wmd_ws_layouts.h"

#pragma clang fp contract(off)

namespace wmd {

constexpr int kInThreads = 256;
constexpr int kMaxScales = 8;

// ---------------------------------------------------------------- the pyramid's plan (host)
struct PyrLevel : ResampleTables {
    int hi, wi, h, w;        // input and output size of the level
    int th, rows;            // tile height, LDS intermediate rows
    size_t lds;              // dynamic LDS bytes
    size_t pix;             // offset of the level in the packed outputs, in pixels (all images)
};

struct PyrPlan {
    int S;
    PyrLevel l[kMaxScales];
    size_t table_ints, pixels;
};

static size_t level_lds(int rows, int ksh, int ksv, int th) { return ((size_t)rows * kTileW * 3 + 3) / 4 * 4 + 4 * ((size_t)kTileW * ksh + (size_t)th * ksv); }

// 0 = ok; otherwise a status, with the message in `why`
static int pyr_plan(int N, int H0, int W0, int height, int width, int S, PyrPlan& p, char* why, size_t why_len) {
    if (N < 1 || H0 < 1 || W0 < 1 || height < 1 || width < 1) {
        snprintf(why, why_len, "N=%d native %dx%d target %dx%d must be positive", N, H0, W0, height, width);
        return WMD_ERR_BAD_SHAPE;
    }
    if (S < 1 || S > kMaxScales || (height >> (S - 1)) < 1 || (width >> (S - 1)) < 1) {
        snprintf(why, why_len, "num_scales=%d: 1..%d, and the last level of %dx%d must not be empty", S, kMaxScales, height, width);
        return WMD_ERR_BAD_SHAPE;
    }
    if (H0 > kMaxDim || W0 > kMaxDim || height > kMaxDim || width > kMaxDim || N > 65535) {
        snprintf(why, why_len, "sizes above %d (or N above 65535) are not implemented", kMaxDim);
        return WMD_ERR_UNSUPPORTED;
    }
    p.S = S;
    p.table_ints = p.pixels = 0;
    int hi = H0, wi = W0;
    for (int s = 0; s < S; ++s) {
        PyrLevel& l = p.l[s];
        l.hi = hi;
        l.wi = wi;
        l.h = height >> s;
        l.w = width >> s;
        l.place(WMD_FILTER_LANCZOS, wi, l.w, hi, l.h, p.table_ints);
        l.pix = p.pixels;
        p.pixels += (size_t)N * l.h * l.w;
        l.th = fit_tile_height([&](int th) {
            l.rows = resample_span(WMD_FILTER_LANCZOS, hi, l.h, th);
            return l.lds = level_lds(l.rows, l.ksh, l.ksv, th);
        });
        if (l.th == 0) {
            snprintf(why, why_len, "level %d (%dx%d -> %dx%d) needs %zu bytes of LDS for one output row", s, hi, wi, l.h, l.w, l.lds);
            return WMD_ERR_UNSUPPORTED;
        }
        hi = l.h;
        wi = l.w;
    }
    return WMD_OK;
}

// ---------------------------------------------------------------- device: colour jitter
struct JitterArgs {   // device arrays, one entry per image; enable == nullptr: no jitter at all
    const unsigned char* enable;
    const unsigned char* order;   // [N,4]
    const float* factors;         // [N,3]
    const int* hue_shift;         // [N]
};

struct JitterItem {
    int on, order[4], shift;
    float f[3];
};

__device__ __forceinline__ JitterItem jitter_load(const JitterArgs& a, size_t n) {
    JitterItem j;
    j.on = a.enable != nullptr && a.enable[n] != 0;
    if (j.on) {
#pragma unroll
        for (int k = 0; k < 4; ++k) j.order[k] = a.order[4 * n + k] & 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) j.f[k] = a.factors[3 * n + k];
        j.shift = a.hue_shift[n] & 255;
    }
    return j;
}

// ImagingBlend(deg, img, f) on one channel: float32, product and sum rounded apart, truncated
__device__ __forceinline__ int blend1(int deg, int img, float f, bool inside) {
    const float prod = f * (float)(img - deg);
    float o = (float)deg + prod;
    if (!inside) o = o <= 0.f ? 0.f : (o >= 255.f ? 255.f : o);
    return (int)o;
}

__device__ __forceinline__ int grey_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Convert.c rgb2hsv_row, H += shift, hsv2rgb
__device__ __forceinline__ void hue_op(int& r, int& g, int& b, int shift) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int H = 0, S = 0;
    const int V = mx;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = cr / (float)mx;
        const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
        float h;   // the sums in double, rounded to float32 once
        if (r == mx) h = (float)((double)bc - (double)gc);
        else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        double hd = (double)h / 6.0 + 1.0;   // in (0.8, 1.9): fmod(hd, 1.0) = hd - floor(hd), exactly
        hd = hd - floor(hd);
        const float hf = (float)hd;
        H = clip8((int)((double)hf * 255.0));
        S = clip8((int)((double)s * 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) {
        r = g = b = V;
        return;
    }
    const float hf = (float)H * 6.0f / 255.0f;
    const float fi = floorf(hf);
    const float f = hf - fi;
    const float fs = (float)S / 255.0f;
    const float v = (float)V;
    const int p = clip8((int)floorf(v * (1.0f - fs) + 0.5f));
    const int q = clip8((int)floorf(v * (1.0f - fs * f) + 0.5f));
    const int t = clip8((int)floorf(v * (1.0f - fs * (1.0f - f)) + 0.5f));
    switch ((int)fi % 6) {
        case 0: r = V; g = t; b = p; break;
        case 1: r = q; g = V; b = p; break;
        case 2: r = p; g = V; b = t; break;
        case 3: r = p; g = q; b = V; break;
        case 4: r = t; g = p; b = V; break;
        default: r = V; g = p; b = q; break;
    }
}

// The ops of one item in order.  kUntilContrast: stop in front of the contrast op -- the pixel whose grey value the mean is
// taken over; otherwise the whole chain with that mean.
template <bool kUntilContrast>
__device__ __forceinline__ void jitter_chain(int& r, int& g, int& b, const JitterItem& j, int mean) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = j.order[k];
        if (op == 3) {
            hue_op(r, g, b, j.shift);
            continue;
        }
        if (op == 1 && kUntilContrast) return;
        const float f = op == 0 ? j.f[0] : (op == 1 ? j.f[1] : j.f[2]);   // no dynamic index: the item stays in registers
        const bool inside = f >= 0.f && f <= 1.f;
        const int gr = grey_of(r, g, b);
        const int dr = op == 0 ? 0 : (op == 1 ? mean : gr);
        r = blend1(dr, r, f, inside);
        g = blend1(dr, g, f, inside);
        b = blend1(dr, b, f, inside);
    }
}

// adds the block's `v` to *dst (one global atomic per block)
__device__ __forceinline__ void block_add(unsigned long long v, unsigned long long* dst) {
    __shared__ unsigned long long acc;
    if (threadIdx.x == 0) acc = 0ull;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&acc, v);
    __syncthreads();
    if (threadIdx.x == 0 && acc) atomicAdd(dst, acc);
}

// ---------------------------------------------------------------- device: one pyramid level
struct ResizeArgs {
    const unsigned char* src;   // [N,hi,wi,3]
    unsigned char* dst;         // [N,h,w,3]
    const int *hb, *hk, *vb, *vk;
    int hi, wi, h, w, ksh, ksv, th, rows;
    const unsigned char* flip;  // level 0 only, may be null
    JitterArgs jit;
    unsigned long long* sums;   // [N] of this level, may be null
};

__global__ __launch_bounds__(kInThreads) void resize_level_kernel(ResizeArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned char* mid = lds_raw;                                                     // [rows][64][3]
    int* hk_s = (int*)(lds_raw + ((size_t)a.rows * kTileW * 3 + 3) / 4 * 4);          // [ksh][64]
    int* vk_s = hk_s + (size_t)kTileW * a.ksh;                                        // [th][ksv]
    const int tid = threadIdx.x, lane = tid & (kTileW - 1), wave = tid / kTileW;
    const size_t n = blockIdx.z;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * a.th;
    const int ncols = min(kTileW, a.w - x0), nrow_out = min(a.th, a.h - y0);
    const bool hpass = a.wi != a.w, vpass = a.hi != a.h;
    // the tile's input rows [row_lo, row_lo + nrows), never more than the LDS holds and never outside the image
    int row_lo, nrows;
    tile_window(a.vb, vpass, y0, nrow_out, a.hi, a.rows, row_lo, nrows);
    // this thread's column of the horizontal pass
    int xmin = 0, xn = 0;
    if (lane < ncols) {
        if (hpass) {
            tap_window(a.hb, x0 + lane, a.ksh, 0, a.wi, xmin, xn);
            stage_hk(hk_s, a.hk, a.ksh, x0 + lane, lane);
        } else {
            xmin = x0 + lane;   // <= w - 1 = wi - 1
            xn = 1;
        }
    }
    if (vpass) stage_vk(vk_s, a.vk, a.ksv, y0, nrow_out, tid, kInThreads);
    __syncthreads();
    const bool flip = a.flip != nullptr && a.flip[n] != 0;
    const unsigned char* img = a.src + n * (size_t)a.hi * a.wi * 3;
    const int xs = 3 * (flip ? a.wi - 1 - xmin : xmin), step = flip ? -3 : 3;   // flipped: from the mirrored column backwards
    for (int rr = wave; rr < nrows; rr += kInThreads / kTileW) {
        if (lane >= ncols) continue;
        const unsigned char* row = img + (size_t)(row_lo + rr) * a.wi * 3 + xs;
        int px[3];
        if (hpass) {
            resample_taps<3>(px, hk_s + lane, kTileW, row, step, xn);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = row[c];
        }
        unsigned char* m = mid + ((size_t)rr * kTileW + lane) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = (unsigned char)px[c];
    }
    __syncthreads();
    const JitterItem jit = jitter_load(a.jit, n);
    unsigned long long grey_sum = 0ull;
    unsigned char* out = a.dst + n * (size_t)a.h * a.w * 3;
    for (int ry = wave; ry < nrow_out; ry += kInThreads / kTileW) {
        if (lane >= ncols) continue;
        const int y = y0 + ry;
        int px[3];
        if (vpass) {
            int ymin, yn;
            tap_window(a.vb, y, a.ksv, row_lo, nrows, ymin, yn);
            resample_taps<3>(px, vk_s + ry * a.ksv, 1, mid + ((size_t)ymin * kTileW + lane) * 3, kTileW * 3, yn);
        } else {
            const unsigned char* m = mid + ((size_t)ry * kTileW + lane) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = ry < nrows ? (int)m[c] : 0;
        }
        unsigned char* o = out + ((size_t)y * a.w + x0 + lane) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (unsigned char)px[c];
        if (jit.on) {
            jitter_chain<true>(px[0], px[1], px[2], jit, 0);
            grey_sum += (unsigned)grey_of(px[0], px[1], px[2]);
        }
    }
    if (a.sums != nullptr && jit.on) block_add(grey_sum, a.sums + n);   // jit.on is uniform over the block
}

// ---------------------------------------------------------------- device: ToTensor + jitter over all levels
struct FinishArgs {
    int levels, N;
    int hw[kMaxScales];
    size_t pix[kMaxScales];             // offset of the level in src / color / aug, in pixels
    const unsigned char* src;           // packed uint8 levels, HWC
    float *color, *aug;                 // kToFloat: packed CHW levels (aug may be null)
    unsigned char* out_u8;              // !kToFloat: jittered uint8, HWC
    JitterArgs jit;
    const unsigned long long* sums;     // [levels][N]
};

template <bool kToFloat>
__global__ __launch_bounds__(kInThreads) void finish_kernel(FinishArgs a) {
    const int s = blockIdx.z;
    const size_t n = blockIdx.y;
    const size_t hw = (size_t)a.hw[s];
    const size_t base = a.pix[s] + n * hw;
    const JitterItem jit = jitter_load(a.jit, n);
    int mean = 0;
    if (jit.on) {
        const unsigned long long sum = a.sums[(size_t)s * a.N + n];
        mean = (int)((2ull * sum + hw) / (2ull * hw));
    }
    for (size_t i = (size_t)blockIdx.x * kInThreads + threadIdx.x; i < hw; i += (size_t)gridDim.x * kInThreads) {
        const unsigned char* px = a.src + (base + i) * 3;
        int r = px[0], g = px[1], b = px[2];
        if (kToFloat) {
            float* c = a.color + base * 3 + i;
            c[0] = (float)r / 255.0f;
            c[hw] = (float)g / 255.0f;
            c[2 * hw] = (float)b / 255.0f;
            if (a.aug == nullptr) continue;
        }
        if (jit.on) jitter_chain<false>(r, g, b, jit, mean);
        if (kToFloat) {
            float* c = a.aug + base * 3 + i;
            c[0] = (float)r / 255.0f;
            c[hw] = (float)g / 255.0f;
            c[2 * hw] = (float)b / 255.0f;
        } else {
            unsigned char* o = a.out_u8 + (base + i) * 3;
            o[0] = (unsigned char)r;
            o[1] = (unsigned char)g;
            o[2] = (unsigned char)b;
        }
    }
}

__global__ __launch_bounds__(kInThreads) void jitter_sum_kernel(const unsigned char* __restrict__ src, size_t hw, JitterArgs jargs,
                                                                unsigned long long* __restrict__ sums) {
    const size_t n = blockIdx.y;
    const JitterItem jit = jitter_load(jargs, n);
    if (!jit.on) return;   // uniform over the block
    unsigned long long grey_sum = 0ull;
    for (size_t i = (size_t)blockIdx.x * kInThreads + threadIdx.x; i < hw; i += (size_t)gridDim.x * kInThreads) {
        const unsigned char* px = src + (n * hw + i) * 3;
        int r = px[0], g = px[1], b = px[2];
        jitter_chain<true>(r, g, b, jit, 0);
        grey_sum += (unsigned)grey_of(r, g, b);
    }
    block_add(grey_sum, sums + n);
}

static unsigned finish_blocks(size_t hw) { return (unsigned)std::min<size_t>((size_t)kNumCU * 8, (hw + kInThreads - 1) / kInThreads); }

}  // namespace wmd

using namespace wmd;

extern "C" int wmd_lanczos_ksize(int in, int out) { return resample_ksize(WMD_FILTER_LANCZOS, in, out); }

extern "C" int wmd_lanczos_table(int in, int out, int* bounds, int* coeffs, int ksize) {
    return resample_table_checked("wmd_lanczos_table", WMD_FILTER_LANCZOS, in, out, bounds, coeffs, ksize);
}

extern "C" size_t wmd_color_pyramid_table_ints(int H0, int W0, int height, int width, int num_scales) {
    PyrPlan p;
    char why[256];
    return pyr_plan(1, H0, W0, height, width, num_scales, p, why, sizeof(why)) == WMD_OK ? p.table_ints : 0;
}

extern "C" int wmd_color_pyramid_tables(int H0, int W0, int height, int width, int num_scales, int* tables, size_t table_ints) {
    const char* who = "wmd_color_pyramid_tables";
    if (!tables) return fail(WMD_ERR_BAD_ARG, "%s: null table pointer", who);
    PyrPlan p;
    char why[256];
    const int st = pyr_plan(1, H0, W0, height, width, num_scales, p, why, sizeof(why));
    if (st != WMD_OK) return fail(st, "%s: %s", who, why);
    if (table_ints != p.table_ints) return fail(WMD_ERR_BAD_ARG, "%s: table_ints=%zu, %zu needed", who, table_ints, p.table_ints);
    for (int s = 0; s < p.S; ++s) {
        const PyrLevel& l = p.l[s];
        l.fill(WMD_FILTER_LANCZOS, l.wi, l.w, l.hi, l.h, tables);
    }
    return WMD_OK;
}

extern "C" size_t wmd_color_pyramid_workspace_bytes(int N, int H0, int W0, int height, int width, int num_scales) {
    PyrPlan p;
    char why[256];
    return pyr_plan(N, H0, W0, height, width, num_scales, p, why, sizeof(why)) == WMD_OK ? array_layout<unsigned long long>(nullptr, (size_t)p.S * N).bytes : 0;
}

static int jitter_args(const char* who, const unsigned char* enable, const unsigned char* order, const float* factors, const int* hue_shift,
                       JitterArgs& j) {
    if (enable && (!order || !factors || !hue_shift)) return fail(WMD_ERR_BAD_ARG, "%s: null jitter parameter pointer (enable is given)", who);
    j.enable = enable;
    j.order = order;
    j.factors = factors;
    j.hue_shift = hue_shift;
    return WMD_OK;
}

extern "C" int wmd_color_pyramid(const unsigned char* frames, int N, int H0, int W0, int height, int width, int num_scales,
                                 const unsigned char* flip, const unsigned char* enable, const unsigned char* order, const float* factors,
                                 const int* hue_shift, const int* tables, unsigned char* levels, float* color, float* color_aug,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "wmd_color_pyramid";
    if (!frames || !tables || !levels || !color) return fail(WMD_ERR_BAD_ARG, "%s: null tensor pointer", who);
    JitterArgs jit;
    if (int st = jitter_args(who, enable, order, factors, hue_shift, jit)) return st;
    if (enable && !color_aug) return fail(WMD_ERR_BAD_ARG, "%s: null color_aug with jitter parameters", who);
    PyrPlan p;
    char why[256];
    if (int st = pyr_plan(N, H0, W0, height, width, num_scales, p, why, sizeof(why))) return fail(st, "%s: %s", who, why);
    const size_t need = array_layout<unsigned long long>(nullptr, (size_t)p.S * N).bytes;
    if (int st = check_workspace(who, workspace, workspace_bytes, need, 8, WMD_ERR_WORKSPACE)) return st;
    unsigned long long* sums = array_layout<unsigned long long>(workspace, (size_t)p.S * N).p;
    hipStream_t s = (hipStream_t)stream;
    if (enable) {
        hipError_t e = hipMemsetAsync(sums, 0, need, s);
        if (e != hipSuccess) return fail(WMD_ERR_HIP, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    }
    FinishArgs f = {};
    f.levels = p.S;
    f.N = N;
    int max_hw = 0;
    for (int k = 0; k < p.S; ++k) {
        const PyrLevel& l = p.l[k];
        ResizeArgs a;
        a.src = k == 0 ? frames : levels + p.l[k - 1].pix * 3;
        a.dst = levels + l.pix * 3;
        a.hb = tables + l.hb;
        a.hk = tables + l.hk;
        a.vb = tables + l.vb;
        a.vk = tables + l.vk;
        a.hi = l.hi; a.wi = l.wi; a.h = l.h; a.w = l.w; a.ksh = l.ksh; a.ksv = l.ksv; a.th = l.th; a.rows = l.rows;
        a.flip = k == 0 ? flip : nullptr;
        a.jit = jit;
        a.sums = enable ? sums + (size_t)k * N : nullptr;
        const double px_in = (double)N * l.hi * l.wi, px_out = (double)N * l.h * l.w;
        ProfScope prof("resize_level_kernel", 2.0 * 3.0 * (px_out * l.ksv + px_in * l.w / l.wi * l.ksh), 3.0 * (px_in + px_out), s);
        hipLaunchKernelGGL(resize_level_kernel, dim3((l.w + kTileW - 1) / kTileW, (l.h + l.th - 1) / l.th, N), dim3(kInThreads), l.lds, s, a);
        f.hw[k] = l.h * l.w;
        f.pix[k] = l.pix;
        max_hw = std::max(max_hw, l.h * l.w);
    }
    f.src = levels;
    f.color = color;
    f.aug = color_aug;
    f.jit = jit;
    f.sums = sums;
    {
        ProfScope prof("finish_kernel", 0.0, (double)p.pixels * 3.0 * (1.0 + (color_aug ? 8.0 : 4.0)), s);
        hipLaunchKernelGGL(finish_kernel<true>, dim3(finish_blocks(max_hw), N, p.S), dim3(kInThreads), 0, s, f);
    }
    return check_launch("color pyramid kernels");
}

static bool jitter_shape_ok(int N, int h, int w) { return N >= 1 && h >= 1 && w >= 1; }
static bool jitter_shape_supported(int N, int h, int w) { return N <= 65535 && (double)h * w < 2147483648.0; }

extern "C" size_t wmd_color_jitter_workspace_bytes(int N, int h, int w) {
    return jitter_shape_ok(N, h, w) && jitter_shape_supported(N, h, w) ? array_layout<unsigned long long>(nullptr, N).bytes : 0;
}

extern "C" int wmd_color_jitter(const unsigned char* images, unsigned char* out, int N, int h, int w, const unsigned char* enable,
                                const unsigned char* order, const float* factors, const int* hue_shift, void* workspace,
                                size_t workspace_bytes, void* stream) {
    const char* who = "wmd_color_jitter";
    if (!images || !out || !enable) return fail(WMD_ERR_BAD_ARG, "%s: null tensor pointer", who);
    JitterArgs jit;
    if (int st = jitter_args(who, enable, order, factors, hue_shift, jit)) return st;
    if (!jitter_shape_ok(N, h, w)) return fail(WMD_ERR_BAD_SHAPE, "%s: N=%d h=%d w=%d must be positive", who, N, h, w);
    if (!jitter_shape_supported(N, h, w)) return fail(WMD_ERR_UNSUPPORTED, "%s: N=%d above 65535 or h*w=%.0f at or above 2^31", who, N, (double)h * w);
    const size_t need = wmd_color_jitter_workspace_bytes(N, h, w);
    if (int st = check_workspace(who, workspace, workspace_bytes, need, 8, WMD_ERR_WORKSPACE)) return st;
    unsigned long long* sums = array_layout<unsigned long long>(workspace, N).p;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(sums, 0, need, s);
    if (e != hipSuccess) return fail(WMD_ERR_HIP, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    const size_t hw = (size_t)h * w;
    const double px = (double)N * hw;
    {
        ProfScope prof("jitter_sum_kernel", 0.0, 3.0 * px, s);
        hipLaunchKernelGGL(jitter_sum_kernel, dim3(finish_blocks(hw), N), dim3(kInThreads), 0, s, images, hw, jit, sums);
    }
    FinishArgs f = {};
    f.levels = 1;
    f.N = N;
    f.hw[0] = (int)hw;
    f.src = images;
    f.out_u8 = out;
    f.jit = jit;
    f.sums = sums;
    {
        ProfScope prof("finish_kernel", 0.0, 6.0 * px, s);
        hipLaunchKernelGGL(finish_kernel<false>, dim3(finish_blocks(hw), N, 1), dim3(kInThreads), 0, s, f);
    }
    return check_launch("color jitter kernels");
}
