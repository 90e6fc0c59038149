// NYUv2 training inputs (NYUv2/data.py, getDefaultTrainTransform / getNoTransform): B decoded uint8 images [B,H0,W0,3] and 8-bit
// depth maps [B,H0,W0] -> image float32 [B,3,ih,iw] and depth float32 [B,1,dh,dw] (optionally 10 / depth and the uint8 resized
// planes), bit for bit what the reference's chain gives over Pillow: flip, channel swap, the gamma table, crop, Pillow's 8-bit
// bicubic resize, ToTensor, * 1000 and the clamp.  Integer and float32 arithmetic with every operation rounded on its own, hence
// the file-wide `fp contract(off)` (wmd_inputs.hip says why).
//
//   wmd_resample.h          the bicubic tables (host; they depend on (in, out) only), the fixed-point pass and its clamped windows
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
#include <stdint.h>
#include <algorithm>
#include "wmd_internal.h"
#include "wmd_resample.h"

#pragma clang fp contract(off)

namespace wmd {
namespace {

constexpr int kNyuThreads = 256;
constexpr int kNyuWaves = kNyuThreads / kTileW;

// ---------------------------------------------------------------- the call's plan (host)
struct NyuPlane : ResampleTables {   // the image or the depth map: (Hs, Ws) -> (h, w), C bytes per pixel
    int C, h, w;
    int th, rows, cols;      // tile height; source rows and source columns a tile reads, at most
    int stride;              // bytes of one staged source row in LDS, a multiple of 4
    unsigned off_mid, off_hk, off_vk, off_lut;   // byte offsets into the dynamic LDS
    size_t lds;
    int tiles_x, tiles_y;
};

struct NyuPlan {
    int Hs, Ws;              // the crop box
    NyuPlane p[2];           // 0 image, 1 depth
    size_t table_ints, lds;
};

void plane_lds(NyuPlane& l) {
    l.stride = (l.cols * l.C + 3) / 4 * 4;
    size_t o = (size_t)l.rows * l.stride;
    l.off_mid = (unsigned)o;
    o += ((size_t)l.rows * kTileW * l.C + 3) / 4 * 4;
    l.off_hk = (unsigned)o;
    o += 4 * (size_t)kTileW * l.ksh;
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
    if (H0 > kMaxDim || W0 > kMaxDim || ih > kMaxDim || iw > kMaxDim || dh > kMaxDim || dw > kMaxDim || B > 65535) {
        snprintf(why, why_len, "sizes above %d (or B above 65535) are not implemented", kMaxDim);
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
        l.place(WMD_FILTER_BICUBIC, p.Ws, l.w, p.Hs, l.h, p.table_ints);
        l.cols = resample_span(WMD_FILTER_BICUBIC, p.Ws, l.w, kTileW);
        l.th = fit_tile_height([&](int th) {
            l.th = th;
            l.rows = resample_span(WMD_FILTER_BICUBIC, p.Hs, l.h, th);
            plane_lds(l);
            return l.lds;
        });
        if (l.th == 0) {
            snprintf(why, why_len, "%s (%dx%d -> %dx%d) needs %zu bytes of LDS for one output row", k == 0 ? "image" : "depth", p.Hs, p.Ws, l.h,
                     l.w, l.lds);
            return WMD_ERR_UNSUPPORTED;
        }
        l.tiles_x = (l.w + kTileW - 1) / kTileW;
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
    const int tid = threadIdx.x, lane = tid & (kTileW - 1), wave = tid / kTileW;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int x0 = tx * kTileW, y0 = ty * a.th;
    const int ncols = min(kTileW, a.w - x0), nrow_out = min(a.th, a.h - y0);
    const bool hpass = g.Ws != a.w, vpass = g.Hs != a.h;
    // the tile's source rows [row_lo, row_lo + nrows) and columns [col_lo, col_lo + ncs) inside the crop box: never more than
    // the LDS holds and never outside the box
    int row_lo, nrows, col_lo, ncs;
    tile_window(a.vb, vpass, y0, nrow_out, g.Hs, a.rows, row_lo, nrows);
    tile_window(a.hb, hpass, x0, ncols, g.Ws, a.cols, col_lo, ncs);
    // this thread's column of the horizontal pass, relative to col_lo
    int xmin = 0, xn = 0;
    if (lane < ncols) {
        if (hpass) {
            tap_window(a.hb, x0 + lane, a.ksh, col_lo, ncs, xmin, xn);
            stage_hk(hk_s, a.hk, a.ksh, x0 + lane, lane);
        } else {
            xmin = lane;
            xn = lane < ncs ? 1 : 0;
        }
    }
    if (vpass) stage_vk(vk_s, a.vk, a.ksv, y0, nrow_out, tid, kNyuThreads);
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
            resample_taps<C>(acc, hk_s + lane, kTileW, s, C, xn);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = xn ? (int)s[c] : 0;
        }
        unsigned char* m = mid + ((size_t)rr * kTileW + lane) * C;
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
            int ymin, yn;
            tap_window(a.vb, y, a.ksv, row_lo, nrows, ymin, yn);
            resample_taps<C>(acc, vk_s + ry * a.ksv, 1, mid + ((size_t)ymin * kTileW + lane) * C, kTileW * C, yn);
        } else {
            const unsigned char* m = mid + ((size_t)ry * kTileW + lane) * C;
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
    return resample_table_checked("wmd_resample_table", filter, in, out, bounds, coeffs, ksize);
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
    for (int k = 0; k < 2; ++k) p.p[k].fill(WMD_FILTER_BICUBIC, p.Ws, p.p[k].w, p.Hs, p.p[k].h, tables);
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
