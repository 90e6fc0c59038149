// NYUv2 training inputs (NYUv2/data.py, getDefaultTrainTransform / getNoTransform): B decoded uint8 images [B,H0,W0,3] and 8-bit
// depth maps [B,H0,W0] -> image float32 [B,3,ih,iw] and depth float32 [B,1,dh,dw] (optionally 10 / depth and the uint8 resized
// planes), bit for bit what the reference's chain gives over Pillow: flip, channel swap, the gamma table, crop, Pillow's 8-bit
// bicubic resize, ToTensor, * 1000 and the clamp.  Integer and float32 arithmetic with every operation rounded on its own, hence
// the file-wide `fp contract(off)` (wmd_inputs.hip says why).
//
//   resample_table (host)   Resample.c precompute_coeffs + normalize_coeffs_8bpc in double for the bicubic (a = -0.5, support 2)
//                           and the Lanczos (support 3) filter; depends on (filter, in, out) only
//   nyu_inputs_kernel       ONE launch per call.  A block owns 64 x th output pixels of one image or of one depth map (the grid's
//                           x axis lists the image tiles, then the depth tiles).  It stages the tile's source footprint -- the rows
//                           of its vertical window times the columns of its horizontal window, inside the crop box -- in LDS,
//                           then runs the horizontal pass from LDS into a uint8 LDS intermediate, the vertical pass from the
//                           intermediate, and the float32 epilogue with planar stores.
//
// Crop, flip, channel permutation and the 256-entry table all happen while staging, so both passes are plain: the crop is an
// offset, the flip a mirrored source column (the fixed-point tables are not mirror symmetric, so flipping the result would
// differ), the permutation and the table apply to source pixels before the filter, as in the reference, image only.
//
// Staging reads aligned dwords wherever the dword lies wholly inside the row span being staged (which lies inside the tensor)
// and single bytes for the ragged head and tail: a row of 3 W0 or W0 bytes starts on any byte address.  No load touches a byte
// outside the input tensors.  Every index that comes out of a device-side table or parameter array is clamped to the tensor
// or LDS region it addresses.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "wmd_internal.h"

#pragma clang fp contract(off)

namespace wmd {
namespace {

constexpr int kNyuThreads = 256;
constexpr int kNyuTileW = 64;         // one wave per intermediate / output row of a tile
constexpr int kNyuMaxTileH = 16;
constexpr int kNyuMaxDim = 32768;
constexpr size_t kNyuMaxLds = 48 * 1024;
constexpr int kNyuPrecisionBits = 32 - 8 - 2;
constexpr int kNyuWaves = kNyuThreads / kNyuTileW;

// ---------------------------------------------------------------- host: coefficient tables
double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

double lanczos3_filter(double x) {
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

bool filter_ok(int filter) { return filter == WMD_FILTER_BICUBIC || filter == WMD_FILTER_LANCZOS; }
double filter_support(int filter) { return filter == WMD_FILTER_BICUBIC ? 2.0 : 3.0; }

int resample_ksize(int filter, int in, int out) {
    if (!filter_ok(filter) || in < 1 || out < 1 || in > kNyuMaxDim || out > kNyuMaxDim) return 0;
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(filter_support(filter) * fs) * 2 + 1;
}

void resample_bound(int filter, int in, int out, int xx, int* xmin, int* n, double* center_out = nullptr) {
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
void resample_table(int filter, int in, int out, int ksize, int* bounds, int* coeffs) {
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, ss = 1.0 / fs;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out; ++xx) {
        int xmin, n;
        double center;
        resample_bound(filter, in, out, xx, &xmin, &n, &center);
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            const double t = (x + xmin - center + 0.5) * ss;
            k[x] = filter == WMD_FILTER_BICUBIC ? bicubic_filter(t) : lanczos3_filter(t);
            ww += k[x];
        }
        int* c = coeffs + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            if (x >= n) {
                c[x] = 0;
                continue;
            }
            const double w = ww != 0.0 ? k[x] / ww : k[x];
            c[x] = w < 0 ? (int)(-0.5 + w * (1 << kNyuPrecisionBits)) : (int)(0.5 + w * (1 << kNyuPrecisionBits));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
}

// ---------------------------------------------------------------- the call's plan (host)
struct NyuPlane {            // the image or the depth map: (Hs, Ws) -> (h, w), C bytes per pixel
    int C, h, w;
    int ksh, ksv;            // table row lengths; a pass is skipped where in == out (Pillow skips it too)
    int th, rows, cols;      // tile height; source rows and source columns a tile reads, at most
    int stride;              // bytes of one staged source row in LDS, a multiple of 4
    unsigned off_mid, off_hk, off_vk, off_lut;   // byte offsets into the dynamic LDS
    size_t lds;
    size_t hb, hk, vb, vk;   // offsets into the table, in ints
    int tiles_x, tiles_y;
};

struct NyuPlan {
    int Hs, Ws;              // the crop box
    NyuPlane p[2];           // 0 image, 1 depth
    size_t table_ints, lds;
};

// the longest source span that `t` outputs starting at any tile boundary read
int worst_span(int in, int out, int t) {
    if (in == out) return std::min(t, out);
    int worst = 0;
    for (int o = 0; o < out; o += t) {
        int lo, n0, last_min, n1;
        resample_bound(WMD_FILTER_BICUBIC, in, out, o, &lo, &n0);
        resample_bound(WMD_FILTER_BICUBIC, in, out, std::min(o + t, out) - 1, &last_min, &n1);
        worst = std::max(worst, last_min + n1 - lo);
    }
    return worst;
}

void plane_lds(NyuPlane& l) {
    l.stride = (l.cols * l.C + 3) / 4 * 4;
    size_t o = (size_t)l.rows * l.stride;
    l.off_mid = (unsigned)o;
    o += ((size_t)l.rows * kNyuTileW * l.C + 3) / 4 * 4;
    l.off_hk = (unsigned)o;
    o += 4 * (size_t)kNyuTileW * l.ksh;
    l.off_vk = (unsigned)o;
    o += 4 * (size_t)l.th * l.ksv;
    l.off_lut = (unsigned)o;
    o += l.C == 3 ? 256 : 0;
    l.lds = o;
}

// 0 = ok; otherwise a status, with the message in `why`
int nyu_plan(int B, int H0, int W0, int crop, int ih, int iw, int dh, int dw, NyuPlan& p, char* why, size_t why_len) {
    if (B < 1 || H0 < 1 || W0 < 1 || ih < 1 || iw < 1 || dh < 1 || dw < 1 || crop < 0) {
        snprintf(why, why_len, "B=%d native %dx%d crop %d image %dx%d depth %dx%d: sizes must be positive, crop not negative", B, H0, W0, crop, ih, iw,
                 dh, dw);
        return WMD_ERR_BAD_SHAPE;
    }
    if (2 * (long long)crop >= H0 || 2 * (long long)crop >= W0) {
        snprintf(why, why_len, "crop=%d leaves nothing of %dx%d", crop, H0, W0);
        return WMD_ERR_BAD_SHAPE;
    }
    if (H0 > kNyuMaxDim || W0 > kNyuMaxDim || ih > kNyuMaxDim || iw > kNyuMaxDim || dh > kNyuMaxDim || dw > kNyuMaxDim || B > 65535) {
        snprintf(why, why_len, "sizes above %d (or B above 65535) are not implemented", kNyuMaxDim);
        return WMD_ERR_UNSUPPORTED;
    }
    p.Hs = H0 - 2 * crop;
    p.Ws = W0 - 2 * crop;
    p.table_ints = 0;
    p.lds = 0;
    for (int k = 0; k < 2; ++k) {
        NyuPlane& l = p.p[k];
        l.C = k == 0 ? 3 : 1;
        l.h = k == 0 ? ih : dh;
        l.w = k == 0 ? iw : dw;
        l.ksh = resample_ksize(WMD_FILTER_BICUBIC, p.Ws, l.w);
        l.ksv = resample_ksize(WMD_FILTER_BICUBIC, p.Hs, l.h);
        l.hb = p.table_ints;
        l.hk = l.hb + 2 * (size_t)l.w;
        l.vb = l.hk + (size_t)l.w * l.ksh;
        l.vk = l.vb + 2 * (size_t)l.h;
        p.table_ints = l.vk + (size_t)l.h * l.ksv;
        l.cols = worst_span(p.Ws, l.w, kNyuTileW);
        for (l.th = kNyuMaxTileH;; l.th /= 2) {
            l.rows = worst_span(p.Hs, l.h, l.th);
            plane_lds(l);
            if (l.lds <= kNyuMaxLds) break;
            if (l.th == 1) {
                snprintf(why, why_len, "%s (%dx%d -> %dx%d) needs %zu bytes of LDS for one output row", k == 0 ? "image" : "depth", p.Hs, p.Ws, l.h,
                         l.w, l.lds);
                return WMD_ERR_UNSUPPORTED;
            }
        }
        l.tiles_x = (l.w + kNyuTileW - 1) / kNyuTileW;
        l.tiles_y = (l.h + l.th - 1) / l.th;
        if ((long long)l.tiles_x * l.tiles_y > (1ll << 30)) {
            snprintf(why, why_len, "%dx%d output: too many tiles for one launch", l.h, l.w);
            return WMD_ERR_UNSUPPORTED;
        }
        p.lds = std::max(p.lds, l.lds);
    }
    return WMD_OK;
}

// ---------------------------------------------------------------- device
struct PlaneArgs {
    const unsigned char* src;   // [B,H0,W0,C]
    float* out;                 // [B,C,h,w]
    float* disp;                // depth only, may be null
    unsigned char* out_u8;      // [B,h,w,C], may be null
    const int *hb, *hk, *vb, *vk;
    int h, w, ksh, ksv, th, rows, cols, stride, tiles_x, tiles;
    unsigned off_mid, off_hk, off_vk, off_lut;
};

struct NyuArgs {
    PlaneArgs img, dep;
    int H0, W0, crop, Hs, Ws;
    const unsigned char *flip, *perm, *lut;   // [B], [B], [B,256]; each may be null
};

__device__ __forceinline__ int nyu_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one source byte, `j` bytes into the staged span of a row, to its place in LDS: pixel mirrored, channel permuted, value mapped
template <int C>
__device__ __forceinline__ void stage_byte(unsigned char* row_s, int j, int v, int ncs, bool flip, int inv_perm, const unsigned char* lut_s) {
    int px = j / C, ch = j - px * C;
    if (flip) px = ncs - 1 - px;
    if (C == 3) {
        ch = (inv_perm >> (4 * ch)) & 3;
        if (lut_s != nullptr) v = lut_s[v];
    }
    row_s[px * C + ch] = (unsigned char)v;
}

template <int C>
__device__ __forceinline__ void nyu_tile(const NyuArgs& g, const PlaneArgs& a, unsigned char* lds, int tile, size_t n) {
    unsigned char* src_s = lds;                                  // [rows][stride]
    unsigned char* mid = lds + a.off_mid;                        // [rows][64][C]
    int* hk_s = (int*)(lds + a.off_hk);                          // [ksh][64]
    int* vk_s = (int*)(lds + a.off_vk);                          // [th][ksv]
    unsigned char* lut_s = lds + a.off_lut;                      // [256], image only
    const int tid = threadIdx.x, lane = tid & (kNyuTileW - 1), wave = tid / kNyuTileW;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * kNyuTileW, y0 = ty * a.th;
    const int ncols = min(kNyuTileW, a.w - x0), nrow_out = min(a.th, a.h - y0);
    const bool hpass = g.Ws != a.w, vpass = g.Hs != a.h;
    // the tile's source rows [row_lo, row_lo + nrows) and columns [col_lo, col_lo + ncs) inside the crop box: never more than
    // the LDS holds and never outside the box
    int row_lo = y0, nrows = nrow_out;
    if (vpass) {
        row_lo = min(max(a.vb[2 * y0], 0), g.Hs);
        const int last = y0 + nrow_out - 1;
        nrows = min(max(a.vb[2 * last] + a.vb[2 * last + 1], row_lo), g.Hs) - row_lo;
    }
    nrows = min(min(nrows, a.rows), g.Hs - row_lo);
    int col_lo = x0, ncs = ncols;
    if (hpass) {
        col_lo = min(max(a.hb[2 * x0], 0), g.Ws);
        const int last = x0 + ncols - 1;
        ncs = min(max(a.hb[2 * last] + a.hb[2 * last + 1], col_lo), g.Ws) - col_lo;
    }
    ncs = min(min(ncs, a.cols), g.Ws - col_lo);
    // this thread's column of the horizontal pass, relative to col_lo
    int xmin = 0, xn = 0;
    if (lane < ncols) {
        if (hpass) {
            xmin = min(max(a.hb[2 * (x0 + lane)], col_lo), col_lo + ncs);
            xn = min(max(a.hb[2 * (x0 + lane) + 1], 0), min(a.ksh, col_lo + ncs - xmin));
            xmin -= col_lo;
            for (int t = 0; t < a.ksh; ++t) hk_s[t * kNyuTileW + lane] = a.hk[(size_t)(x0 + lane) * a.ksh + t];
        } else {
            xmin = lane;
            xn = lane < ncs ? 1 : 0;
        }
    }
    if (vpass)
        for (int i = tid; i < nrow_out * a.ksv; i += kNyuThreads) vk_s[i] = a.vk[(size_t)y0 * a.ksv + i];
    const bool flip = g.flip != nullptr && g.flip[n] != 0;
    int inv_perm = 0x210;
    bool table = false;
    if (C == 3) {
        if (g.perm != nullptr) {
            // nibble k of the code is perm[k], in the order of itertools.permutations(range(3)); out[k] = in[perm[k]]
            const int q = min((int)g.perm[n], 5);
            const int code = q == 0 ? 0x210 : (q == 1 ? 0x120 : (q == 2 ? 0x201 : (q == 3 ? 0x021 : (q == 4 ? 0x102 : 0x012))));
            inv_perm = (0 << (4 * (code & 3))) | (1 << (4 * ((code >> 4) & 3))) | (2 << (4 * ((code >> 8) & 3)));
        }
        table = g.lut != nullptr;
        if (table) lut_s[tid] = g.lut[n * 256 + tid];            // kNyuThreads == 256
        __syncthreads();
    }
    // ---- stage: per row the span of ncs pixels, mirrored within the crop box where flipped
    {
        const int xs = g.crop + (flip ? g.Ws - col_lo - ncs : col_lo);   // first source column of the span, in the native row
        const int len = ncs * C;
        const int units = len / 4 + 7;                                   // per row: up to 3 head bytes, the dwords, up to 3 tail bytes
        const unsigned char* base = a.src + ((n * (size_t)g.H0 + (size_t)(g.crop + row_lo)) * g.W0 + xs) * C;
        for (int i = tid; i < nrows * units; i += kNyuThreads) {
            const int r = i / units, u = i - r * units;
            const unsigned char* p = base + (size_t)r * g.W0 * C;
            const int head = min((int)((0 - (uintptr_t)p) & 3), len);
            const int ndw = (len - head) / 4, tail = len - head - 4 * ndw;
            unsigned char* row_s = src_s + (size_t)r * a.stride;
            const unsigned char* lut_p = table ? lut_s : nullptr;
            if (u < head) {
                stage_byte<C>(row_s, u, p[u], ncs, flip, inv_perm, lut_p);
            } else if (u < head + ndw) {
                const int j = head + 4 * (u - head);
                const unsigned v = *(const unsigned*)(p + j);            // aligned, and wholly inside [p, p + len)
#pragma unroll
                for (int k = 0; k < 4; ++k) stage_byte<C>(row_s, j + k, (v >> (8 * k)) & 255, ncs, flip, inv_perm, lut_p);
            } else if (u < head + ndw + tail) {
                const int j = head + 4 * ndw + (u - head - ndw);
                stage_byte<C>(row_s, j, p[j], ncs, flip, inv_perm, lut_p);
            }
        }
    }
    __syncthreads();
    // ---- horizontal pass: LDS -> uint8 LDS intermediate
    for (int rr = wave; rr < nrows; rr += kNyuWaves) {
        if (lane >= ncols) continue;
        const unsigned char* s = src_s + (size_t)rr * a.stride + xmin * C;
        int acc[C];
        if (hpass) {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 1 << (kNyuPrecisionBits - 1);
            for (int t = 0; t < xn; ++t) {
                const int k = hk_s[t * kNyuTileW + lane];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += k * (int)s[t * C + c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = nyu_clip8(acc[c] >> kNyuPrecisionBits);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = xn ? (int)s[c] : 0;
        }
        unsigned char* m = mid + ((size_t)rr * kNyuTileW + lane) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) m[c] = (unsigned char)acc[c];
    }
    __syncthreads();
    // ---- vertical pass and the float32 epilogue
    const size_t hw = (size_t)a.h * a.w;
    for (int ry = wave; ry < nrow_out; ry += kNyuWaves) {
        if (lane >= ncols) continue;
        const int y = y0 + ry;
        int acc[C];
        if (vpass) {
            int ymin = min(max(a.vb[2 * y], row_lo), row_lo + nrows);
            const int yn = min(max(a.vb[2 * y + 1], 0), min(a.ksv, row_lo + nrows - ymin));
            ymin -= row_lo;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 1 << (kNyuPrecisionBits - 1);
            for (int t = 0; t < yn; ++t) {
                const int k = vk_s[ry * a.ksv + t];
                const unsigned char* m = mid + ((size_t)(ymin + t) * kNyuTileW + lane) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += k * (int)m[c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = nyu_clip8(acc[c] >> kNyuPrecisionBits);
        } else {
            const unsigned char* m = mid + ((size_t)ry * kNyuTileW + lane) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = ry < nrows ? (int)m[c] : 0;
        }
        const size_t pix = (size_t)y * a.w + x0 + lane;
        if (a.out_u8 != nullptr) {
            unsigned char* o = a.out_u8 + (n * hw + pix) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = (unsigned char)acc[c];
        }
        float* o = a.out + n * hw * C + pix;
        if (C == 3) {
#pragma unroll
            for (int c = 0; c < C; ++c) o[c * hw] = (float)acc[c] / 255.0f;
        } else {
            const float d = fminf(fmaxf(((float)acc[0] / 255.0f) * 1000.0f, 10.0f), 1000.0f);
            o[0] = d;
            if (a.disp != nullptr) a.disp[n * hw + pix] = 10.0f / d;
        }
    }
}

__global__ __launch_bounds__(kNyuThreads) void nyu_inputs_kernel(NyuArgs g) {
    extern __shared__ __align__(16) unsigned char nyu_lds[];
    const size_t n = blockIdx.y;
    const int tile = blockIdx.x;           // uniform over the block
    if (tile < g.img.tiles)
        nyu_tile<3>(g, g.img, nyu_lds, tile, n);
    else
        nyu_tile<1>(g, g.dep, nyu_lds, tile - g.img.tiles, n);
}

void plane_args(const NyuPlane& l, const int* tables, PlaneArgs& a) {
    a.hb = tables + l.hb;
    a.hk = tables + l.hk;
    a.vb = tables + l.vb;
    a.vk = tables + l.vk;
    a.h = l.h; a.w = l.w; a.ksh = l.ksh; a.ksv = l.ksv; a.th = l.th; a.rows = l.rows; a.cols = l.cols; a.stride = l.stride;
    a.tiles_x = l.tiles_x;
    a.tiles = l.tiles_x * l.tiles_y;
    a.off_mid = l.off_mid; a.off_hk = l.off_hk; a.off_vk = l.off_vk; a.off_lut = l.off_lut;
}

}  // namespace
}  // namespace wmd

using namespace wmd;

extern "C" int wmd_resample_ksize(int filter, int in, int out) { return resample_ksize(filter, in, out); }

extern "C" int wmd_resample_table(int filter, int in, int out, int* bounds, int* coeffs, int ksize) {
    const char* who = "wmd_resample_table";
    if (!bounds || !coeffs) return fail(WMD_ERR_BAD_ARG, "%s: null table pointer", who);
    if (!filter_ok(filter)) return fail(WMD_ERR_BAD_ARG, "%s: filter=%d is neither WMD_FILTER_BICUBIC nor WMD_FILTER_LANCZOS", who, filter);
    const int need = resample_ksize(filter, in, out);
    if (need == 0) return fail(WMD_ERR_BAD_SHAPE, "%s: in=%d out=%d must be in 1..%d", who, in, out, kNyuMaxDim);
    if (ksize != need) return fail(WMD_ERR_BAD_ARG, "%s: ksize=%d, wmd_resample_ksize(%d, %d, %d) = %d", who, ksize, filter, in, out, need);
    resample_table(filter, in, out, ksize, bounds, coeffs);
    return WMD_OK;
}

extern "C" size_t wmd_nyu_inputs_table_ints(int H0, int W0, int crop, int ih, int iw, int dh, int dw) {
    NyuPlan p;
    char why[256];
    return nyu_plan(1, H0, W0, crop, ih, iw, dh, dw, p, why, sizeof(why)) == WMD_OK ? p.table_ints : 0;
}

extern "C" int wmd_nyu_inputs_tables(int H0, int W0, int crop, int ih, int iw, int dh, int dw, int* tables, size_t table_ints) {
    const char* who = "wmd_nyu_inputs_tables";
    if (!tables) return fail(WMD_ERR_BAD_ARG, "%s: null table pointer", who);
    NyuPlan p;
    char why[256];
    const int st = nyu_plan(1, H0, W0, crop, ih, iw, dh, dw, p, why, sizeof(why));
    if (st != WMD_OK) return fail(st, "%s: %s", who, why);
    if (table_ints != p.table_ints) return fail(WMD_ERR_BAD_ARG, "%s: table_ints=%zu, %zu needed", who, table_ints, p.table_ints);
    for (int k = 0; k < 2; ++k) {
        const NyuPlane& l = p.p[k];
        resample_table(WMD_FILTER_BICUBIC, p.Ws, l.w, l.ksh, tables + l.hb, tables + l.hk);
        resample_table(WMD_FILTER_BICUBIC, p.Hs, l.h, l.ksv, tables + l.vb, tables + l.vk);
    }
    return WMD_OK;
}

extern "C" int wmd_nyu_inputs(const unsigned char* image_u8, const unsigned char* depth_u8, int B, int H0, int W0, int crop, int ih, int iw,
                              int dh, int dw, const unsigned char* flip, const unsigned char* perm, const unsigned char* lut,
                              const int* tables, size_t table_ints, float* image, float* depth, float* disp_gt,
                              unsigned char* image_resized, unsigned char* depth_resized, void* stream) {
    const char* who = "wmd_nyu_inputs";
    if (!image_u8 || !depth_u8 || !tables || !image || !depth) return fail(WMD_ERR_BAD_ARG, "%s: null tensor pointer", who);
    if ((size_t)tables & 3) return fail(WMD_ERR_BAD_ARG, "%s: tables at %p is not 4-byte aligned", who, (const void*)tables);
    NyuPlan p;
    char why[256];
    if (int st = nyu_plan(B, H0, W0, crop, ih, iw, dh, dw, p, why, sizeof(why))) return fail(st, "%s: %s", who, why);
    if (table_ints != p.table_ints)
        return fail(WMD_ERR_BAD_ARG, "%s: table_ints=%zu, wmd_nyu_inputs_table_ints gives %zu for this shape", who, table_ints, p.table_ints);
    hipStream_t s = (hipStream_t)stream;
    NyuArgs g = {};
    plane_args(p.p[0], tables, g.img);
    plane_args(p.p[1], tables, g.dep);
    g.img.src = image_u8;
    g.img.out = image;
    g.img.out_u8 = image_resized;
    g.dep.src = depth_u8;
    g.dep.out = depth;
    g.dep.disp = disp_gt;
    g.dep.out_u8 = depth_resized;
    g.H0 = H0; g.W0 = W0; g.crop = crop; g.Hs = p.Hs; g.Ws = p.Ws;
    g.flip = flip;
    g.perm = perm;
    g.lut = lut;
    const double px_in = (double)B * p.Hs * p.Ws, px_img = (double)B * ih * iw, px_dep = (double)B * dh * dw;
    double flops = 0.0;
    for (int k = 0; k < 2; ++k) {
        const NyuPlane& l = p.p[k];
        flops += 2.0 * l.C * B * ((double)l.h * l.w * l.ksv + (double)p.Hs * l.w * l.ksh);
    }
    const double bytes = 4.0 * px_in + px_img * (12.0 + (image_resized ? 3.0 : 0.0)) + px_dep * (4.0 + (disp_gt ? 4.0 : 0.0) + (depth_resized ? 1.0 : 0.0));
    {
        ProfScope prof("nyu_inputs_kernel", flops, bytes, s);
        hipLaunchKernelGGL(nyu_inputs_kernel, dim3(g.img.tiles + g.dep.tiles, B), dim3(kNyuThreads), p.lds, s, g);
    }
    return check_launch("nyu_inputs_kernel");
}
