// Pillow's 8-bit resample (Resample.c precompute_coeffs + normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc), the one
// core of wmd_inputs.hip and wmd_nyu_inputs.hip: the coefficient tables on the host, the fixed-point pass and the clamped
// windows on the device.  The tables are double arithmetic that must equal Pillow's x86 build, which has no fused
// multiply-add; hipcc contracts a * b + c by default, hence the pragma, which this header sets for itself.
#pragma once
#include <math.h>
#include <algorithm>
#include <vector>
#include "wmd_internal.h"

#pragma clang fp contract(off)

namespace wmd {

constexpr int kTileW = 64;          // one wave per intermediate / output row of a tile
constexpr int kMaxTileH = 16;
constexpr int kMaxDim = 32768;
constexpr size_t kMaxLds = 48 * 1024;
constexpr int kPrecisionBits = 32 - 8 - 2;

// ---------------------------------------------------------------- host: coefficient tables
static double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

static double lanczos_filter(double x) {
    if (-3.0 <= x && x < 3.0) {
        auto sinc = [](double t) {
            if (t == 0.0) return 1.0;
            t = t * M_PI;
            return sin(t) / t;
        };
        return sinc(x) * sinc(x / 3);
    }
    return 0.0;
}

static bool filter_ok(int filter) { return filter == WMD_FILTER_BICUBIC || filter == WMD_FILTER_LANCZOS; }
static double filter_support(int filter) { return filter == WMD_FILTER_BICUBIC ? 2.0 : 3.0; }

static int resample_ksize(int filter, int in, int out) {
    if (!filter_ok(filter) || in < 1 || out < 1 || in > kMaxDim || out > kMaxDim) return 0;
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(filter_support(filter) * fs) * 2 + 1;
}

static void resample_bound(int filter, int in, int out, int xx, int* xmin, int* n, double* center_out = nullptr) {
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, support = filter_support(filter) * fs;
    const double center = (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > in) hi = in;
    *xmin = lo;
    *n = hi - lo;
    if (center_out) *center_out = center;
}

// bounds [out][2] = (xmin, n), coeffs [out][ksize] (zero beyond n)
static void resample_table(int filter, int in, int out, int ksize, int* bounds, int* coeffs) {
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, ss = 1.0 / fs;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out; ++xx) {
        int xmin, n;
        double center;
        resample_bound(filter, in, out, xx, &xmin, &n, &center);
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            const double t = (x + xmin - center + 0.5) * ss;
            k[x] = filter == WMD_FILTER_BICUBIC ? bicubic_filter(t) : lanczos_filter(t);
            ww += k[x];
        }
        int* c = coeffs + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            if (x >= n) {
                c[x] = 0;
                continue;
            }
            const double w = ww != 0.0 ? k[x] / ww : k[x];
            c[x] = w < 0 ? (int)(-0.5 + w * (1 << kPrecisionBits)) : (int)(0.5 + w * (1 << kPrecisionBits));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
}

// wmd_lanczos_table / wmd_resample_table under the entry point's name `who`: the refusals, then the table
static int resample_table_checked(const char* who, int filter, int in, int out, int* bounds, int* coeffs, int ksize) {
    if (!bounds || !coeffs) return fail(WMD_ERR_BAD_ARG, "%s: null table pointer", who);
    if (!filter_ok(filter)) return fail(WMD_ERR_BAD_ARG, "%s: filter=%d is neither WMD_FILTER_BICUBIC nor WMD_FILTER_LANCZOS", who, filter);
    const int need = resample_ksize(filter, in, out);
    if (need == 0) return fail(WMD_ERR_BAD_SHAPE, "%s: in=%d out=%d must be in 1..%d", who, in, out, kMaxDim);
    if (ksize != need) return fail(WMD_ERR_BAD_ARG, "%s: ksize=%d, %d needed for filter=%d in=%d out=%d", who, ksize, need, filter, in, out);
    resample_table(filter, in, out, ksize, bounds, coeffs);
    return WMD_OK;
}

// the longest source span that `t` outputs starting at any tile boundary read
static int resample_span(int filter, int in, int out, int t) {
    if (in == out) return std::min(t, out);
    int worst = 0;
    for (int o = 0; o < out; o += t) {
        int lo, n0, last_min, n1;
        resample_bound(filter, in, out, o, &lo, &n0);
        resample_bound(filter, in, out, std::min(o + t, out) - 1, &last_min, &n1);
        worst = std::max(worst, last_min + n1 - lo);
    }
    return worst;
}

// the largest tile height, a power of two up to kMaxTileH, whose LDS request `lds_of(th)` fits; 0: one output row does not
template <class F>
static int fit_tile_height(F lds_of) {
    for (int th = kMaxTileH; th >= 1; th /= 2)
        if (lds_of(th) <= kMaxLds) return th;
    return 0;
}

// The tables of one pass pair, horizontal wi -> w then vertical hi -> h, in the caller's table of ints: (bounds, coeffs) of
// the width, then of the height.
struct ResampleTables {
    int ksh, ksv;            // table row lengths; a pass is skipped where in == out (Pillow skips it too)
    size_t hb, hk, vb, vk;   // offsets into the table, in ints

    void place(int filter, int wi, int w, int hi, int h, size_t& table_ints) {   // appends at the running `table_ints`
        ksh = resample_ksize(filter, wi, w);
        ksv = resample_ksize(filter, hi, h);
        hb = table_ints;
        hk = hb + 2 * (size_t)w;
        vb = hk + (size_t)w * ksh;
        vk = vb + 2 * (size_t)h;
        table_ints = vk + (size_t)h * ksv;
    }
    void fill(int filter, int wi, int w, int hi, int h, int* tables) const {
        resample_table(filter, wi, w, ksh, tables + hb, tables + hk);
        resample_table(filter, hi, h, ksv, tables + vb, tables + vk);
    }
};

// ---------------------------------------------------------------- device: the fixed-point pass
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one output pixel of a pass: acc[c] = clip8(((1 << 21) + sum_t k[t kstride] src[t sstride + c]) >> 22) in int32.  sstride is
// signed: a mirrored gather walks the source backwards.
template <int C>
__device__ __forceinline__ void resample_taps(int (&acc)[C], const int* k, int kstride, const unsigned char* src, int sstride, int n) {
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < n; ++t) {
        const int kt = k[t * kstride];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += kt * (int)src[t * sstride + c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = clip8(acc[c] >> kPrecisionBits);
}

// the coefficients of a tile into LDS: output column `col`'s row of hk as column `lane` of hk_s [ksh][64] (one call per lane),
// rows y0 .. y0 + nrow_out - 1 of vk as vk_s [nrow_out][ksv] (the whole block of `threads`)
__device__ __forceinline__ void stage_hk(int* hk_s, const int* hk, int ksh, int col, int lane) {
    for (int t = 0; t < ksh; ++t) hk_s[t * kTileW + lane] = hk[(size_t)col * ksh + t];
}
__device__ __forceinline__ void stage_vk(int* vk_s, const int* vk, int ksv, int y0, int nrow_out, int tid, int threads) {
    for (int i = tid; i < nrow_out * ksv; i += threads) vk_s[i] = vk[(size_t)y0 * ksv + i];
}

// Every index that comes out of a device-side table is clamped to what it addresses:
// the source span [lo, lo + n) of outputs o0 .. o0 + cnt - 1 by the bounds table `b` (`pass` off: the outputs themselves),
// never outside [0, in) and never longer than `cap`, what the LDS holds
__device__ __forceinline__ void tile_window(const int* b, bool pass, int o0, int cnt, int in, int cap, int& lo, int& n) {
    lo = o0;
    n = cnt;
    if (pass) {
        lo = min(max(b[2 * o0], 0), in);
        const int last = o0 + cnt - 1;
        n = min(max(b[2 * last] + b[2 * last + 1], lo), in) - lo;
    }
    n = min(min(n, cap), in - lo);
}
// the taps of output `o` inside the window [lo, lo + n): the first one relative to lo, and how many (at most ks)
__device__ __forceinline__ void tap_window(const int* b, int o, int ks, int lo, int n, int& first, int& taps) {
    const int mn = min(max(b[2 * o], lo), lo + n);
    taps = min(max(b[2 * o + 1], 0), min(ks, lo + n - mn));
    first = mn - lo;
}

}  // namespace wmd
