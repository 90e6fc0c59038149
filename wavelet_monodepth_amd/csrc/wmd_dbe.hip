// Depth-boundary errors of the NYUv2 evaluation: NYUv2/utils.py:122-169
// compute_depth_boundary_error, the two columns dbe_acc / dbe_com that NYUv2/evaluate.py:94-107 prints with --eval_edges.
// The reference copies one prediction per loop iteration to the host and runs skimage's Canny and two scipy distance
// transforms there; here a batch stays in HBM and nothing is read back, not even inside the hysteresis:
//   dbe_init_kernel      per-image state: min / max keys, counters, two distance histograms
//   dbe_prep_kernel      NaN-aware min and max of the non-zero depths (order-preserving integer keys: exact and
//                        order-free), ground-truth edges packed to bit planes (one ballot per 64 columns), their count
//   dbe_smooth_kernel    normalise (0 -> NaN, - min, / max) + separable Gaussian in float64 over 16 x 64 tiles with a
//                        `radius` halo staged in LDS; zeros outside the image; divided by the filtered all-ones image
//   dbe_nms_kernel       Sobel pair (mirrored borders), hypot, non-maximum suppression with the interpolated neighbours,
//                        the two thresholds; weak / strong pixels leave as bit planes
//   dbe_hyst_kernel      hysteresis: one workgroup per image holds the weak and the marked plane bit-packed in LDS and
//                        sweeps under workgroup barriers until a sweep changes nothing (at most H W sweeps) -- no
//                        grid-wide synchronisation, no host loop.  The marked plane only grows and its fixed point (the
//                        weak components that hold a strong pixel) is unique, so the result does not depend on timing.
//   dbe_chamfer_kernel   at every edge pixel the squared distance to the nearest edge of the other map, searched over the
//                        21 x 21 neighbourhood of the bit planes (only distances below 10 count: exact); integer
//                        histograms over the squared distance 0..99 and ">= 100"
//   dbe_finish_kernel    the two scores from the histograms, summed in a fixed order in float64: deterministic
// The detector is this project's definition, modelled on skimage.feature.canny(image, sigma, low, high) with mask=None
// (see include/wmd.h); all of its arithmetic is float64.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "wmd_internal.h"
#include "wmd_select.h"
#include "wmd_ws_layouts.h"

namespace wmd {

constexpr int DBE_MAX_RADIUS = 12;              // Gaussian taps 2 * 12 + 1: sigma up to 3.1
constexpr int DBE_TH = 16, DBE_TW = 64;         // tile of the smoothing and suppression kernels: one wavefront per row
constexpr int DBE_PLANE_WORDS = 16384;          // 64 KiB of LDS per bit plane in the hysteresis (two planes)
constexpr int DBE_HA = 4, DBE_HB = 105, DBE_NBIN = 101;
constexpr double DBE_EPS = 2.220446049250313e-16;

struct DbeTaps {
    double w[2 * DBE_MAX_RADIUS + 1];
    int radius;
};

__global__ void dbe_init_kernel(unsigned* __restrict__ state, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) state[i] = (i % DBE_STATE == 0) ? 0xFFFFFFFFu : 0u;
}

// one wavefront per (row, 64-column segment)
__global__ __launch_bounds__(256) void dbe_prep_kernel(const float* __restrict__ pred, const unsigned char* __restrict__ gt,
                                                       unsigned* __restrict__ gt_plane, unsigned* __restrict__ state,
                                                       int H, int W, int Wp) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int nseg = Wp >> 1, items = H * nseg;
    const size_t plane = (size_t)H * W;
    KeyRange<true> kr;
    unsigned ngt = 0;
    for (int it = blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += gridDim.x * 4) {
        const int r = it / nseg, sg = it - r * nseg, c = sg * 64 + lane;
        const bool in = c < W;
        const float v = in ? pred[b * plane + (size_t)r * W + c] : 0.f;
        if (v != 0.f && v == v) kr.take(order_key(v));
        const bool g = in && gt[b * plane + (size_t)r * W + c] != 0;
        const unsigned long long bits = __ballot(g);
        if (lane == 0) {
            unsigned* p = gt_plane + ((size_t)b * H + r) * Wp + sg * 2;
            p[0] = (unsigned)bits;
            p[1] = (unsigned)(bits >> 32);
            ngt += __popcll(bits);
        }
    }
    kr.wave();                 // a wave publishes for itself: its lane 0 also holds the edge count of its rows
    if (lane == 0) {
        unsigned* st = state + (size_t)b * DBE_STATE;
        if (kr.mn != 0xFFFFFFFFu) {
            atomicMin(&st[0], kr.mn);
            atomicMax(&st[1], kr.mx);
        }
        if (ngt) atomicAdd(&st[3], ngt);
    }
}

// smoothed = G(p) / (G(ones) + eps), zeros outside the image.  normalise != 0: p = (img == 0 ? NaN : img - min) / (max - min)
// with the image's keys from dbe_prep_kernel (no valid pixel: the keys decode to NaN; a constant image: 0 / 0).
__global__ __launch_bounds__(256) void dbe_smooth_kernel(const float* __restrict__ img, const unsigned* __restrict__ state,
                                                         double* __restrict__ sm, int H, int W, DbeTaps taps, int normalise) {
    extern __shared__ double dbe_lds[];
    const int R = taps.radius, IW = DBE_TW + 2 * R, IH = DBE_TH + 2 * R;
    double* tin = dbe_lds;                 // [IH][IW]
    double* tv = dbe_lds + IH * IW;        // [DBE_TH][IW]
    const int b = blockIdx.z, y0 = blockIdx.y * DBE_TH, x0 = blockIdx.x * DBE_TW;
    const float* src = img + (size_t)b * H * W;
    double mn = 0.0, range = 1.0;
    if (normalise) {
        mn = (double)order_unkey(state[(size_t)b * DBE_STATE + 0]);
        range = (double)order_unkey(state[(size_t)b * DBE_STATE + 1]) - mn;
    }
    for (int i = threadIdx.x; i < IH * IW; i += 256) {
        const int rr = i / IW, cc = i - rr * IW, y = y0 - R + rr, x = x0 - R + cc;
        double v = 0.0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const float f = src[(size_t)y * W + x];
            if (normalise) v = f == 0.f ? nan("") : ((double)f - mn) / range;
            else v = (double)f;
        }
        tin[i] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DBE_TH * IW; i += 256) {
        const int r = i / IW, cc = i - r * IW;
        double s = 0.0;
        for (int k = 0; k <= 2 * R; ++k) s += taps.w[k] * tin[(r + k) * IW + cc];
        tv[i] = s;
    }
    __syncthreads();
    const int c = threadIdx.x & 63, x = x0 + c;
    double nx = 0.0;
    for (int k = 0; k <= 2 * R; ++k) nx += (x + k - R >= 0 && x + k - R < W) ? taps.w[k] : 0.0;
    for (int r = threadIdx.x >> 6; r < DBE_TH; r += 4) {
        const int y = y0 + r;
        if (y >= H || x >= W) continue;
        double s = 0.0, ny = 0.0;
        for (int k = 0; k <= 2 * R; ++k) {
            s += taps.w[k] * tv[r * IW + c + k];
            ny += (y + k - R >= 0 && y + k - R < H) ? taps.w[k] : 0.0;
        }
        sm[((size_t)b * H + y) * W + x] = s / (ny * nx + DBE_EPS);
    }
}

// mirror about the edge (d c b a | a b c d), then clamp: positions further out than the image is wide feed only pixels
// outside the image, which are never used
__device__ __forceinline__ int dbe_mirror(int i, int n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

constexpr int DBE_SW = DBE_TW + 4, DBE_MW = DBE_TW + 2;

// Sobel pair at the position whose centre is s[rc][cc]
__device__ __forceinline__ void dbe_sobel(const double* s, int rc, int cc, double& is, double& js) {
    const double* up = s + (rc - 1) * DBE_SW + cc;
    const double* md = s + rc * DBE_SW + cc;
    const double* dn = s + (rc + 1) * DBE_SW + cc;
    is = (dn[-1] - up[-1]) + 2.0 * (dn[0] - up[0]) + (dn[1] - up[1]);
    js = (up[1] - up[-1]) + 2.0 * (md[1] - md[-1]) + (dn[1] - dn[-1]);
}

__global__ __launch_bounds__(256) void dbe_nms_kernel(const double* __restrict__ sm, unsigned* __restrict__ weak_plane,
                                                      unsigned* __restrict__ strong_plane, int H, int W, int Wp, double low,
                                                      double high) {
    __shared__ double s[(DBE_TH + 4) * DBE_SW];      // smoothed, halo 2
    __shared__ double mg[(DBE_TH + 2) * DBE_MW];     // magnitude, halo 1
    const int b = blockIdx.z, y0 = blockIdx.y * DBE_TH, x0 = blockIdx.x * DBE_TW;
    const double* src = sm + (size_t)b * H * W;
    for (int i = threadIdx.x; i < (DBE_TH + 4) * DBE_SW; i += 256) {
        const int rr = i / DBE_SW, cc = i - rr * DBE_SW;
        s[i] = src[(size_t)dbe_mirror(y0 - 2 + rr, H) * W + dbe_mirror(x0 - 2 + cc, W)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (DBE_TH + 2) * DBE_MW; i += 256) {
        const int rr = i / DBE_MW, cc = i - rr * DBE_MW, y = y0 - 1 + rr, x = x0 - 1 + cc;
        double m = 0.0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            double is, js;
            dbe_sobel(s, rr + 1, cc + 1, is, js);
            m = hypot(is, js);
        }
        mg[i] = m;
    }
    __syncthreads();
    const int c = threadIdx.x & 63, x = x0 + c;
    for (int r = threadIdx.x >> 6; r < DBE_TH; r += 4) {
        const int y = y0 + r;
        if (y >= H) break;                                     // uniform over the wavefront
        const double* mc = mg + (r + 1) * DBE_MW + c + 1;
        const double m = *mc;
        double out = 0.0;
        if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2 && m >= low) {
            double is, js;
            dbe_sobel(s, r + 2, c + 2, is, js);
            const double ai = fabs(is), aj = fabs(js);
            const bool c1 = (is >= 0 && js >= 0) || (is <= 0 && js <= 0);
            const bool c2 = (is <= 0 && js >= 0) || (is >= 0 && js <= 0);
            // (row, column) offsets of a and b on the positive side; the negative side is the point reflection
            int ar = 0, ac = 0, br = 0, bc = 0;
            double w = 0.0;
            bool any = true;
            if (c1 && ai > aj) { w = aj / ai; ar = 1; ac = 0; br = 1; bc = 1; }
            else if (c1) { w = ai / aj; ar = 0; ac = 1; br = 1; bc = 1; }
            else if (c2 && ai < aj) { w = ai / aj; ar = 0; ac = 1; br = -1; bc = 1; }
            else if (c2) { w = aj / ai; ar = -1; ac = 0; br = -1; bc = 1; }
            else any = false;
            if (any) {
                const double p = mc[br * DBE_MW + bc] * w + mc[ar * DBE_MW + ac] * (1.0 - w);
                const double n = mc[-br * DBE_MW - bc] * w + mc[-ar * DBE_MW - ac] * (1.0 - w);
                if (p <= m && n <= m) out = m;
            }
        }
        const bool wk = out > 0.0, sg = wk && out >= high;
        const unsigned long long wb = __ballot(wk), sb = __ballot(sg);
        if (c == 0) {
            const size_t o = ((size_t)b * H + y) * Wp + blockIdx.x * 2;
            weak_plane[o] = (unsigned)wb;
            weak_plane[o + 1] = (unsigned)(wb >> 32);
            strong_plane[o] = (unsigned)sb;
            strong_plane[o + 1] = (unsigned)(sb >> 32);
        }
    }
}

// one pass over word (r, j): pull marks from the eight neighbouring words, then fill the runs of the word
__device__ __forceinline__ bool dbe_hyst_step(const unsigned* wk, volatile unsigned* mk, int r, int j, int H, int Wp) {
    const int i = r * Wp + j;
    const unsigned w = wk[i];
    if (!w) return false;
    const unsigned m = mk[i];
    if (m == w) return false;
    const bool up = r > 0, dn = r < H - 1;
    unsigned n = m | (up ? mk[i - Wp] : 0u) | (dn ? mk[i + Wp] : 0u);
    unsigned sp = n | (n << 1) | (n >> 1);
    if (j > 0) sp |= (mk[i - 1] | (up ? mk[i - Wp - 1] : 0u) | (dn ? mk[i + Wp - 1] : 0u)) >> 31;
    if (j < Wp - 1) sp |= (mk[i + 1] | (up ? mk[i - Wp + 1] : 0u) | (dn ? mk[i + Wp + 1] : 0u)) << 31;
    unsigned x = m | (w & sp);
    for (;;) {
        const unsigned y = x | (w & ((x << 1) | (x >> 1)));
        if (y == x) break;
        x = y;
    }
    if (x == m) return false;
    mk[i] = x;                                                 // only this thread writes word i
    return true;
}

// strong_plane holds the strong pixels on entry and the edge map on exit.  state != NULL: an image without ground-truth
// edges gets an empty map (compute_depth_boundary_error's first branch).
__global__ __launch_bounds__(1024) void dbe_hyst_kernel(const unsigned* __restrict__ weak_plane, unsigned* __restrict__ strong_plane,
                                                        unsigned char* __restrict__ edges, const unsigned* __restrict__ state,
                                                        int H, int W, int Wp) {
    __shared__ unsigned wk[DBE_PLANE_WORDS];
    __shared__ unsigned mk[DBE_PLANE_WORDS];
    const int b = blockIdx.x, n = H * Wp, t = threadIdx.x;
    const unsigned* gw = weak_plane + (size_t)b * n;
    unsigned* gs = strong_plane + (size_t)b * n;
    const bool skip = state && state[(size_t)b * DBE_STATE + 3] == 0;
    for (int i = t; i < n; i += 1024) {
        const unsigned w = skip ? 0u : gw[i];
        wk[i] = w;
        mk[i] = gs[i] & w;
    }
    __syncthreads();
    // thread = (word column j, chunk of consecutive rows): a sweep walks the chunk down and back up, so marks travel a
    // whole chunk vertically and a word (and its runs) horizontally per sweep
    const int nchunk = 1024 / Wp;                              // Wp <= 1024 (checked by the host)
    const int rows = (H + nchunk - 1) / nchunk;
    const int j = t % Wp, r_lo = (t / Wp) * rows;
    const int r_hi = (t / Wp) < nchunk ? min(H, r_lo + rows) : 0;
    const long long cap = (long long)H * W;
    for (long long sweep = 0; sweep < cap; ++sweep) {
        bool changed = false;
        for (int r = r_lo; r < r_hi; ++r) changed |= dbe_hyst_step(wk, mk, r, j, H, Wp);
        for (int r = r_hi - 1; r >= r_lo; --r) changed |= dbe_hyst_step(wk, mk, r, j, H, Wp);
        if (!__syncthreads_or(changed ? 1 : 0)) break;
    }
    __syncthreads();
    for (int i = t; i < n; i += 1024) gs[i] = mk[i];
    if (edges) {
        unsigned char* e = edges + (size_t)b * H * W;
        for (int p = t; p < H * W; p += 1024) {
            const int r = p / W, c = p - r * W;
            e[p] = (mk[r * Wp + (c >> 5)] >> (c & 31)) & 1u;
        }
    }
}

// squared distance from (r, c) to the nearest set bit of `plane` within the 21 x 21 neighbourhood; 100 when there is none
// closer than 10
__device__ __forceinline__ int dbe_nearest(const unsigned* __restrict__ plane, int r, int c, int H, int Wp) {
    int best = 100;
    const int start = c - 10, w0 = start >> 5, off = start & 31;     // start >= -10: w0 >= -1
    for (int dy = -10; dy <= 10; ++dy) {
        const int y = r + dy, dy2 = dy * dy;
        if (y < 0 || y >= H || dy2 >= best) continue;
        const unsigned* row = plane + (size_t)y * Wp;
        const unsigned long long lo = (w0 >= 0 && w0 < Wp) ? row[w0] : 0u, hi = (w0 + 1 >= 0 && w0 + 1 < Wp) ? row[w0 + 1] : 0u;
        const unsigned win = (unsigned)(((lo | (hi << 32)) >> off) & 0x1FFFFFu);   // bit k = column c - 10 + k
        if (!win) continue;
        int dx = 11;
        const unsigned rt = win >> 10, lf = win & 0x7FFu;
        if (rt) dx = __ffs(rt) - 1;
        if (lf) dx = min(dx, 10 - (31 - __clz(lf)));
        best = min(best, dy2 + dx * dx);
    }
    return best;
}

// histA: predicted edge pixels inside the mask by squared distance to the ground truth; histB: ground-truth edge pixels by
// squared distance to the prediction; n_est: every predicted edge pixel
__global__ __launch_bounds__(256) void dbe_chamfer_kernel(const unsigned* __restrict__ est_plane, const unsigned* __restrict__ gt_plane,
                                                          const unsigned char* __restrict__ mask, unsigned* __restrict__ state,
                                                          int H, int W, int Wp) {
    __shared__ unsigned hist[2 * DBE_NBIN + 1];
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int nseg = Wp >> 1, items = H * nseg;
    const unsigned* est = est_plane + (size_t)b * H * Wp;
    const unsigned* gt = gt_plane + (size_t)b * H * Wp;
    for (int i = threadIdx.x; i < 2 * DBE_NBIN + 1; i += 256) hist[i] = 0;
    __syncthreads();
    for (int it = blockIdx.x * 4 + (threadIdx.x >> 6); it < items; it += gridDim.x * 4) {
        const int r = it / nseg, sg = it - r * nseg, c = sg * 64 + lane;
        const size_t o = (size_t)r * Wp + sg * 2 + (lane >> 5);
        const bool e = (est[o] >> (lane & 31)) & 1u, g = (gt[o] >> (lane & 31)) & 1u;   // bits past W are zero
        if (e) {
            atomicAdd(&hist[2 * DBE_NBIN], 1u);
            if (!mask || mask[((size_t)b * H + r) * W + c] != 0) atomicAdd(&hist[dbe_nearest(gt, r, c, H, Wp)], 1u);
        }
        if (g) atomicAdd(&hist[DBE_NBIN + dbe_nearest(est, r, c, H, Wp)], 1u);
    }
    __syncthreads();
    unsigned* st = state + (size_t)b * DBE_STATE;
    for (int i = threadIdx.x; i < 2 * DBE_NBIN; i += 256)
        if (hist[i]) atomicAdd(&st[DBE_HA + i], hist[i]);      // DBE_HB == DBE_HA + DBE_NBIN
    if (threadIdx.x == 0 && hist[2 * DBE_NBIN]) atomicAdd(&st[2], hist[2 * DBE_NBIN]);
}

__global__ void dbe_finish_kernel(const unsigned* __restrict__ state, float* __restrict__ out2, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned* st = state + (size_t)b * DBE_STATE;
    double sa = 0.0, sb = 0.0, nf = 0.0, ngt = 0.0;
    for (int k = 0; k < 100; ++k) {
        const double d = sqrt((double)k);
        sa += d * (double)st[DBE_HA + k];
        sb += d * (double)st[DBE_HB + k];
        nf += (double)st[DBE_HA + k];
        ngt += (double)st[DBE_HB + k];
    }
    ngt += (double)st[DBE_HB + 100];
    double acc, com;
    if (ngt == 0.0) acc = com = nan("");
    else if (nf == 0.0) acc = com = 10.0;
    else {
        acc = sa / nf;
        com = (sa + 10.0 * (double)st[DBE_HA + 100] + sb + 10.0 * (double)st[DBE_HB + 100]) / ((double)st[2] + ngt);
    }
    out2[b * 2 + 0] = (float)acc;
    out2[b * 2 + 1] = (float)com;
}

static inline int dbe_wp(int W) { return 2 * ((W + 63) / 64); }

// shape and size rules shared by the two entry points; 0 = fine
static int dbe_check_shape(const char* fn, int B, int H, int W) {
    if (B <= 0 || H < 3 || W < 3) return fail(WMD_ERR_BAD_SHAPE, "%s: B=%d H=%d W=%d (needs B >= 1 and H, W >= 3)", fn, B, H, W);
    if (B > 65535 || dbe_wp(W) > 1024 || (long long)H * dbe_wp(W) > DBE_PLANE_WORDS)
        return fail(WMD_ERR_UNSUPPORTED, "%s: B=%d H=%d W=%d: H * 2 * ceil(W / 64) must not exceed %d (the hysteresis keeps two bit "
                    "planes of an image in LDS), B <= 65535", fn, B, H, W, DBE_PLANE_WORDS);
    return WMD_OK;
}

static int dbe_taps(const char* fn, double sigma, DbeTaps* t) {
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(WMD_ERR_BAD_ARG, "%s: sigma=%g", fn, sigma);
    const int R = (int)(4.0 * sigma + 0.5);
    if (R > DBE_MAX_RADIUS) return fail(WMD_ERR_UNSUPPORTED, "%s: sigma=%g needs a radius of %d taps (at most %d)", fn, sigma, R, DBE_MAX_RADIUS);
    double sum = 0.0;
    for (int k = -R; k <= R; ++k) sum += (t->w[k + R] = std::exp(-0.5 / (sigma * sigma) * (double)(k * k)));
    for (int k = 0; k <= 2 * R; ++k) t->w[k] /= sum;
    t->radius = R;
    return WMD_OK;
}

// prep (optional) -> smooth -> suppression -> hysteresis, on a carved workspace
static int dbe_detect(const char* fn, const float* img, const unsigned char* gt, unsigned char* edges, int B, int H, int W,
                      const DbeTaps& taps, double low, double high, const DbeWs& ws, bool normalise, hipStream_t s) {
    const int Wp = dbe_wp(W);
    const double px = (double)B * H * W;
    const dim3 tiles((W + DBE_TW - 1) / DBE_TW, (H + DBE_TH - 1) / DBE_TH, B);
    if (normalise) {
        ProfScope prof("dbe_prep_kernel", 2.0 * px, 5.0 * px, s);
        const int n = B * DBE_STATE;
        hipLaunchKernelGGL(dbe_init_kernel, dim3((n + 255) / 256), dim3(256), 0, s, ws.state, n);
        const int nblk = std::max(1, std::min((H * (Wp / 2) + 3) / 4, 128));
        hipLaunchKernelGGL(dbe_prep_kernel, dim3(nblk, B), dim3(256), 0, s, img, gt, ws.gt, ws.state, H, W, Wp);
    }
    {
        ProfScope prof("dbe_smooth_kernel", 4.0 * (2 * taps.radius + 1) * px, 12.0 * px, s);
        const int R = taps.radius;
        const size_t lds = sizeof(double) * (size_t)(DBE_TW + 2 * R) * (2 * DBE_TH + 2 * R);
        hipLaunchKernelGGL(dbe_smooth_kernel, tiles, dim3(256), lds, s, img, normalise ? ws.state : (const unsigned*)nullptr, ws.sm, H, W,
                           taps, normalise ? 1 : 0);
    }
    {
        ProfScope prof("dbe_nms_kernel", 40.0 * px, 8.25 * px, s);
        hipLaunchKernelGGL(dbe_nms_kernel, tiles, dim3(256), 0, s, ws.sm, ws.weak, ws.strong, H, W, Wp, low, high);
    }
    {
        ProfScope prof("dbe_hyst_kernel", 0.0, px * (edges ? 1.0 : 0.0) + 12.0 * B * H * Wp, s);
        hipLaunchKernelGGL(dbe_hyst_kernel, dim3(B), dim3(1024), 0, s, ws.weak, ws.strong, edges, normalise ? ws.state : (const unsigned*)nullptr,
                           H, W, Wp);
    }
    return check_launch(fn);
}

}  // namespace wmd

using namespace wmd;

extern "C" size_t wmd_eval_dbe_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H < 3 || W < 3) return 0;
    return dbe_layout(nullptr, B, H, W, dbe_wp(W)).bytes;
}

extern "C" int wmd_eval_canny(const float* img, unsigned char* edges_u8, int B, int H, int W, double sigma, double low, double high,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!img || !edges_u8 || !workspace) return fail(WMD_ERR_BAD_ARG, "wmd_eval_canny: null pointer (img, edges_u8 or workspace)");
    int st = dbe_check_shape("wmd_eval_canny", B, H, W);
    if (st) return st;
    DbeTaps taps;
    st = dbe_taps("wmd_eval_canny", sigma, &taps);
    if (st) return st;
    st = check_workspace("wmd_eval_canny", workspace, workspace_bytes, wmd_eval_dbe_workspace_bytes(B, H, W), 8, WMD_ERR_BAD_ARG);
    if (st) return st;
    const DbeWs ws = dbe_layout(workspace, B, H, W, dbe_wp(W));
    return dbe_detect("wmd_eval_canny", img, nullptr, edges_u8, B, H, W, taps, low, high, ws, false, (hipStream_t)stream);
}

extern "C" int wmd_eval_dbe(const float* pred, const unsigned char* edges_gt_u8, const unsigned char* mask_u8, float* out2,
                            unsigned char* edges_est_u8, int B, int H, int W, double low, double high, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!pred || !edges_gt_u8 || !out2 || !workspace) return fail(WMD_ERR_BAD_ARG, "wmd_eval_dbe: null pointer (pred, edges_gt_u8, out2 or workspace)");
    int st = dbe_check_shape("wmd_eval_dbe", B, H, W);
    if (st) return st;
    st = check_workspace("wmd_eval_dbe", workspace, workspace_bytes, wmd_eval_dbe_workspace_bytes(B, H, W), 8, WMD_ERR_BAD_ARG);
    if (st) return st;
    const DbeWs ws = dbe_layout(workspace, B, H, W, dbe_wp(W));
    DbeTaps taps;
    st = dbe_taps("wmd_eval_dbe", std::sqrt(2.0), &taps);
    if (st) return st;
    hipStream_t s = (hipStream_t)stream;
    st = dbe_detect("wmd_eval_dbe", pred, edges_gt_u8, edges_est_u8, B, H, W, taps, low, high, ws, true, s);
    if (st) return st;
    const int Wp = dbe_wp(W);
    ProfScope prof("dbe_chamfer_kernel", 0.0, 8.0 * B * H * Wp, s);
    const int nblk = std::max(1, std::min((H * (Wp / 2) + 3) / 4, 128));
    hipLaunchKernelGGL(dbe_chamfer_kernel, dim3(nblk, B), dim3(256), 0, s, ws.strong, ws.gt, mask_u8, ws.state, H, W, Wp);
    hipLaunchKernelGGL(dbe_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, ws.state, out2, B);
    return check_launch("wmd_eval_dbe");
}
