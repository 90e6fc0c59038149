// Semi-global stereo matching: the matcher that produces the candidates of depth-hint fusion (wmd_hints.hip).  The contract
// is the integer specification of DESIGN.md ("Semi-global stereo matching"), which follows StereoSGBM's documented parameters
// and stages; tests/stereo_ref.py restates it in numpy and every kernel here matches that bit for bit.  Nothing here has been
// compared with OpenCV itself.
//
// Stages, per group of images (as many as fit the workspace cap; grid z = image of the group):
//   stereo_prep_kernel    uint8 HWC (mirrored when reverse[b]) -> per pixel and channel two packed words {value, lo, hi} of the
//                         prefiltered signal G and of the raw signal I: the half-pixel intervals of the pixel cost
//   stereo_cost_kernel    C[y][xv][d] uint16, d innermost, xv = x - x0 over the valid rectangle.  A block owns TY x 8 pixels:
//                         it stages the prepared rows of both views in LDS (planar, so lanes along d read consecutive words),
//                         computes the pixel costs of the tile plus its ring once into LDS and sums the window from there,
//                         two disparities per thread (packed uint16 pairs: the S bound keeps the halves apart)
//   stereo_path_kernel    one launch per direction, one wavefront per scan line of that direction (rows, columns or diagonals:
//                         every path is an independent chain, so L lives in registers and is never stored), disparity
//                         d = 64 r + lane in register r; ragged lanes hold +inf.  min_k by DPP inside rows of 16 lanes and
//                         four v_readlane across them, d +- 1 by a cross-lane move.  The launch adds L into S; every (y, x, d)
//                         has one owner per launch and launches of one stream run in order: no atomics.  Cost and S of eight
//                         steps are loaded before the eight dependent updates, so the chain waits for memory once per eight.
//   stereo_winner_kernel  one wavefront per pixel: packed (S, d) minimum, uniqueness vote, sub-pixel parabola, and the
//                         right-view map as atomicMin of (minS << 16 | x) per landing column: independent of scheduling
//   stereo_finish_kernel  left-right check against those keys, the invalid left band, the mirror back
//   speckle_*_kernel      connected components by lock-free union-find (atomicMin on the larger root, path halving; global, so a
//                         component that crosses anything converges).  Labels start at the first pixel of the horizontal run
//                         (a ballot per wavefront) and only the leftmost vertical link of a group of parallel links is made:
//                         unions per run, not per pixel.  Sizes by atomicAdd at the root, then the clear
#include <algorithm>
#include <stdint.h>
#include "wmd_internal.h"
#include "wmd_ws_layouts.h"

namespace wmd {

constexpr int kSgmInf = 1 << 28;
constexpr int kCostTX = 8;                         // tile columns of stereo_cost_kernel
constexpr int kCostThreads = 256;
constexpr size_t kCostLdsMax = 60 * 1024;
constexpr int kPathBatch = 8;                      // steps whose loads are issued together
constexpr size_t kStereoGroupCap = (size_t)1 << 30;   // bytes of workspace beyond which images run in several groups

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// minimum over the 64 lanes, in every lane; all 64 lanes must be active
__device__ __forceinline__ int wave_min_i32(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm:[1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm:[2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror: every lane has its row's minimum
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return min(min(a, b), min(c, d));
}

// ---------------------------------------------------------------- prep
__device__ __forceinline__ unsigned pack3(int v, int a, int b) {
    const int lo = min(v, min(a, b)), hi = max(v, max(a, b));
    return (unsigned)v | ((unsigned)lo << 8) | ((unsigned)hi << 16);
}

// grid (ceil(W C / 256), H, 2 G): z = 2 * image of the group + view
__global__ __launch_bounds__(256) void stereo_prep_kernel(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                                                          const uint8_t* __restrict__ reverse, uint2* __restrict__ prep, int b0, int H,
                                                          int W, int C, int cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * C) return;
    const int x = i / C, c = i - x * C, y = blockIdx.y, g = blockIdx.z >> 1, side = blockIdx.z & 1, b = b0 + g;
    const uint8_t* img = (side ? right : left) + (size_t)b * H * W * C;
    const bool rev = reverse && reverse[b];
    auto px = [&](int yy, int xx) {
        yy = clampi(yy, 0, H - 1), xx = clampi(xx, 0, W - 1);
        return (int)img[((size_t)yy * W + (rev ? W - 1 - xx : xx)) * C + c];
    };
    auto grad = [&](int xx) {
        xx = clampi(xx, 0, W - 1);
        const int g3 = (px(y - 1, xx + 1) - px(y - 1, xx - 1)) + 2 * (px(y, xx + 1) - px(y, xx - 1)) + (px(y + 1, xx + 1) - px(y + 1, xx - 1));
        return clampi(g3, -cap, cap) + cap;
    };
    const int g0 = grad(x), gm = grad(x - 1), gp = grad(x + 1);
    const int i0 = px(y, x), im = px(y, x - 1), ip = px(y, x + 1);
    prep[(((size_t)(g * 2 + side) * H + y) * W + x) * C + c] = make_uint2(pack3(g0, (g0 + gm) >> 1, (g0 + gp) >> 1), pack3(i0, (i0 + im) >> 1, (i0 + ip) >> 1));
}

// ---------------------------------------------------------------- cost volume
__device__ __forceinline__ int bt_cost(unsigned l, unsigned r) {
    const int v = l & 255, v0 = (l >> 8) & 255, v1 = (l >> 16) & 255, u = r & 255, u0 = (r >> 8) & 255, u1 = (r >> 16) & 255;
    return min(max(0, max(v - u1, u0 - v)), max(0, max(u - v1, v0 - u)));
}

struct CostTile {
    int rows, LW, RW;
    size_t l_words, r_words, bytes;
};
__host__ __device__ inline CostTile cost_tile(int TY, int r, int C, int D) {
    CostTile t;
    t.rows = TY + 2 * r, t.LW = kCostTX + 2 * r, t.RW = t.LW + D - 1;
    t.l_words = (size_t)t.rows * C * 2 * t.LW, t.r_words = (size_t)t.rows * C * 2 * t.RW;
    t.bytes = 4 * (t.l_words + t.r_words) + 2 * (size_t)t.rows * t.LW * D;
    return t;
}

// grid (ceil(Wv / 8), ceil(H / TY), G); dynamic LDS cost_tile(...).bytes
__global__ __launch_bounds__(kCostThreads) void stereo_cost_kernel(const uint2* __restrict__ prep, uint16_t* __restrict__ cost, int H, int W,
                                                                   int C, int minD, int D, int r, int TY, size_t cost_stride) {
    extern __shared__ uint32_t stereo_smem[];
    const CostTile t = cost_tile(TY, r, C, D);
    uint32_t* Lp = stereo_smem;                      // [rows][C][2][LW]
    uint32_t* Rp = Lp + t.l_words;                   // [rows][C][2][RW]
    uint16_t* pcs = (uint16_t*)(Rp + t.r_words);     // [rows][LW][D]
    const int x0 = minD + D, Wv = W - x0, g = blockIdx.z, tid = threadIdx.x;
    const int xt0 = x0 + blockIdx.x * kCostTX, yt0 = blockIdx.y * TY;
    const int xr_lo = clampi(xt0 - r, x0, W - 1) - minD - (D - 1);   // >= 1
    const uint2* PL = prep + (size_t)(g * 2) * H * W * C;
    const uint2* PR = PL + (size_t)H * W * C;

    for (int i = tid; i < t.rows * t.LW * C; i += kCostThreads) {
        const int c = i % C, q = i / C, cx = q % t.LW, ry = q / t.LW;
        const int y = clampi(yt0 - r + ry, 0, H - 1), x = clampi(xt0 - r + cx, x0, W - 1);
        const uint2 v = PL[((size_t)y * W + x) * C + c];
        Lp[((ry * C + c) * 2 + 0) * t.LW + cx] = v.x;
        Lp[((ry * C + c) * 2 + 1) * t.LW + cx] = v.y;
    }
    for (int i = tid; i < t.rows * t.RW * C; i += kCostThreads) {
        const int c = i % C, q = i / C, col = q % t.RW, ry = q / t.RW;
        const int y = clampi(yt0 - r + ry, 0, H - 1), x = min(xr_lo + col, W - 1);
        const uint2 v = PR[((size_t)y * W + x) * C + c];
        Rp[((ry * C + c) * 2 + 0) * t.RW + col] = v.x;
        Rp[((ry * C + c) * 2 + 1) * t.RW + col] = v.y;
    }
    __syncthreads();
    for (int i = tid; i < t.rows * t.LW * D; i += kCostThreads) {
        const int d = i % D, p = i / D, cx = p % t.LW, ry = p / t.LW;
        const int col = clampi(xt0 - r + cx, x0, W - 1) - minD - d - xr_lo;
        int sum = 0;
        for (int c = 0; c < C; ++c) {
            const uint32_t* lp = Lp + (ry * C + c) * 2 * t.LW + cx;
            const uint32_t* rp = Rp + (ry * C + c) * 2 * t.RW + col;
            sum += bt_cost(lp[0], rp[0]) + (bt_cost(lp[t.LW], rp[t.RW]) >> 2);
        }
        pcs[i] = (uint16_t)sum;
    }
    __syncthreads();
    const int D2 = D >> 1, win = 2 * r + 1;
    const uint32_t* pc2 = (const uint32_t*)pcs;
    uint32_t* out = (uint32_t*)(cost + (size_t)g * cost_stride);
    for (int i = tid; i < TY * kCostTX * D2; i += kCostThreads) {
        const int dd = i % D2, p = i / D2, tx = p % kCostTX, ty = p / kCostTX;
        const int y = yt0 + ty, x = xt0 + tx;
        if (y >= H || x >= W) continue;
        uint32_t sum = 0;
        for (int j = 0; j < win; ++j)
            for (int k = 0; k < win; ++k) sum += pc2[((ty + j) * t.LW + tx + k) * D2 + dd];
        out[((size_t)y * Wv + (x - x0)) * D2 + dd] = sum;
    }
}

// ---------------------------------------------------------------- aggregation
// one wavefront per scan line of the step (sx, sy) = minus the predecessor offset; grid (ceil(lines / 4), 1, G)
template <int NR>
__global__ __launch_bounds__(256) void stereo_path_kernel(const uint16_t* __restrict__ cost, uint16_t* __restrict__ S, int H, int Wv, int D,
                                                          int sx, int sy, int P1, int P2, int first, size_t img_stride) {
    const int lane = threadIdx.x & 63, line = blockIdx.x * 4 + (threadIdx.x >> 6);
    int xs, ys, len, nlines;
    if (sy == 0) {
        nlines = H, ys = line, xs = sx > 0 ? 0 : Wv - 1, len = Wv;
    } else if (sx == 0) {
        nlines = Wv, xs = line, ys = sy > 0 ? 0 : H - 1, len = H;
    } else {
        nlines = Wv + H - 1;
        if (line < Wv) {
            xs = line, ys = sy > 0 ? 0 : H - 1;
        } else {
            const int k = line - Wv + 1;
            xs = sx > 0 ? 0 : Wv - 1, ys = sy > 0 ? k : H - 1 - k;
        }
        len = min(sx > 0 ? Wv - xs : xs + 1, sy > 0 ? H - ys : ys + 1);
    }
    if (line >= nlines) return;   // the whole wavefront leaves: every lane is active below
    cost += (size_t)blockIdx.z * img_stride;
    S += (size_t)blockIdx.z * img_stride;
    const ptrdiff_t step = ((ptrdiff_t)sy * Wv + sx) * D;
    ptrdiff_t off = ((ptrdiff_t)ys * Wv + xs) * D;
    bool live[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) live[r] = r * 64 + lane < D;
    int L[NR], minL = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) L[r] = kSgmInf;

    for (int t0 = 0; t0 < len; t0 += kPathBatch) {
        int c[kPathBatch][NR], s[kPathBatch][NR];
#pragma unroll
        for (int u = 0; u < kPathBatch; ++u)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                c[u][r] = 0, s[u][r] = 0;
                if (t0 + u < len && live[r]) {
                    c[u][r] = cost[off + u * step + r * 64 + lane];
                    if (!first) s[u][r] = S[off + u * step + r * 64 + lane];
                }
            }
#pragma unroll
        for (int u = 0; u < kPathBatch; ++u) {
            if (t0 + u < len) {   // wave-uniform
                if (t0 + u == 0) {
#pragma unroll
                    for (int r = 0; r < NR; ++r) L[r] = live[r] ? c[u][r] : kSgmInf;
                } else {
                    int Ln[NR];
#pragma unroll
                    for (int r = 0; r < NR; ++r) {
                        int below = __shfl_up(L[r], 1), above = __shfl_down(L[r], 1);
                        if (lane == 0) below = kSgmInf;
                        if (lane == 63) above = kSgmInf;
                        if (r > 0) {
                            const int e = __builtin_amdgcn_readlane(L[r - 1], 63);
                            if (lane == 0) below = e;
                        }
                        if (r < NR - 1) {
                            const int e = __builtin_amdgcn_readlane(L[r + 1], 0);
                            if (lane == 63) above = e;
                        }
                        const int m = min(min(L[r], min(below, above) + P1), minL + P2);
                        Ln[r] = live[r] ? c[u][r] + m - minL : kSgmInf;
                    }
#pragma unroll
                    for (int r = 0; r < NR; ++r) L[r] = Ln[r];
                }
                int m = L[0];
#pragma unroll
                for (int r = 1; r < NR; ++r) m = min(m, L[r]);
                minL = wave_min_i32(m);
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    if (live[r]) S[off + u * step + r * 64 + lane] = (uint16_t)(s[u][r] + L[r]);
            }
        }
        off += kPathBatch * step;
    }
}

// ---------------------------------------------------------------- winner
// one wavefront per pixel of the valid rectangle; grid (ceil(H Wv / 4), 1, G)
template <int NR>
__global__ __launch_bounds__(256) void stereo_winner_kernel(const uint16_t* __restrict__ S, int16_t* __restrict__ first_map, unsigned* __restrict__ keys,
                                                            int H, int W, int minD, int D, int uniq, size_t img_stride) {
    const int lane = threadIdx.x & 63, pix = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int x0 = minD + D, Wv = W - x0;
    if (pix >= H * Wv) return;
    const int y = pix / Wv, x = x0 + pix - y * Wv, g = blockIdx.z;
    const uint16_t* Sp = S + (size_t)g * img_stride + (size_t)pix * D;
    int v[NR], key = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int d = r * 64 + lane;
        v[r] = 0;
        if (d < D) {
            v[r] = Sp[d];
            key = min(key, (v[r] << 8) | d);
        }
    }
    key = wave_min_i32(key);
    const int ds = key & 255, minS = key >> 8;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int d = r * 64 + lane;
        if (d < D && abs(d - ds) > 1 && v[r] * (100 - uniq) < minS * 100) bad = true;
    }
    const bool reject = __ballot(bad) != 0;
    if (lane == 0) {
        const int dfull = ds + minD;
        const size_t row = ((size_t)g * H + y) * W;
        atomicMin(&keys[row + x - dfull], ((unsigned)minS << 16) | (unsigned)x);
        int disp = (minD - 1) * 16;
        if (!reject) {
            disp = dfull * 16;
            if (ds > 0 && ds < D - 1) {
                const int a = Sp[ds - 1], c = Sp[ds + 1], den = max(a + c - 2 * minS, 1);
                disp += ((a - c) * 16 + den) / (2 * den);
            }
        }
        first_map[row + x] = (int16_t)disp;
    }
}

// left-right check, the left band and the mirror back; grid (ceil(W / 256), H, G)
__global__ __launch_bounds__(256) void stereo_finish_kernel(const int16_t* __restrict__ first_map, const unsigned* __restrict__ keys,
                                                            const uint8_t* __restrict__ reverse, int16_t* __restrict__ disp, int b0, int H, int W,
                                                            int minD, int D, int tol) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, g = blockIdx.z, b = b0 + g;
    if (x >= W) return;
    const int invalid = (minD - 1) * 16;
    const size_t row = ((size_t)g * H + y) * W;
    int d1 = invalid;
    if (x >= minD + D) {
        d1 = first_map[row + x];
        if (d1 != invalid) {
            auto off = [&](int xx, int dd) {
                if (xx < 0 || xx >= W) return false;
                const unsigned k = keys[row + xx];
                return k != 0xFFFFFFFFu && abs((int)(k & 0xFFFFu) - xx - dd) > tol;
            };
            const int a = d1 >> 4, c = (d1 + 15) >> 4;
            if (off(x - a, a) && off(x - c, c)) d1 = invalid;
        }
    }
    const bool rev = reverse && reverse[b];
    disp[((size_t)b * H + y) * W + (rev ? W - 1 - x : x)] = (int16_t)d1;
}

// ---------------------------------------------------------------- speckles
// Labels point at smaller pixel indices only, so the forest has no cycle whatever the interleaving.  uf_find halves the path
// as it walks (plain stores of an ancestor: a store that overwrites a concurrent hook re-attaches the node to a tree the
// hooking thread goes on to merge, see uf_union), which keeps the chains of one large component short.
__device__ __forceinline__ int uf_find(int* labels, int i) {
    volatile int* L = labels;
    int p = L[i];
    while (p != i) {
        const int g = L[p];
        if (g != p) L[i] = g;
        i = p, p = g;
    }
    return i;
}

__device__ __forceinline__ void uf_union(int* labels, int a, int b) {
    bool done = false;
    while (!done) {
        a = uf_find(labels, a), b = uf_find(labels, b);
        if (a == b) break;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = atomicMin(&labels[a], b);   // a > b: hang the larger root below the smaller
        done = old == a;
        a = old;                                    // a was no root any more: what it pointed at still has to meet b
    }
}

__device__ __forceinline__ bool speckle_joined(int a, int b, int invalid, int max_diff) { return a != invalid && b != invalid && abs(a - b) <= max_diff; }

// label = the first pixel of the horizontal run, as far as the wavefront's 64 consecutive pixels see it: a run that goes on
// to the left of lane 0 is joined there by speckle_merge_kernel.  Whole blocks run (no early return): the ballot needs every lane.
__global__ __launch_bounds__(256) void speckle_init_kernel(const int16_t* __restrict__ disp, int* __restrict__ labels, int* __restrict__ counts, int n, int W,
                                                           int invalid, int max_diff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = i < n;
    const int d = in ? disp[i] : invalid;
    const bool valid = d != invalid;
    const bool first = valid && (i % W == 0 || !speckle_joined(disp[i - 1], d, invalid, max_diff));
    const unsigned long long starts = __ballot(first) & ((2ull << lane) - 1);   // run starts at or below this lane
    if (!in) return;
    labels[i] = valid ? (starts ? i - lane + 63 - __clzll(starts) : i - lane) : -1;
    counts[i] = 0;
}

// horizontal: only where a run crosses into lane 0 of a wavefront's span.  vertical: the link (i, i + W) follows from its left
// neighbour's when the two pixels to the left are linked to each other and to these two, so only the leftmost link of such a
// group is made: unions per run, not per pixel.
__global__ __launch_bounds__(256) void speckle_merge_kernel(const int16_t* __restrict__ disp, int* __restrict__ labels, int n, int H, int W, int invalid,
                                                            int max_diff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int d = disp[i];
    if (d == invalid) return;
    const int x = i % W, y = (i / W) % H;
    const bool left = x > 0 && speckle_joined(disp[i - 1], d, invalid, max_diff);
    if (left && (threadIdx.x & 63) == 0) uf_union(labels, i, i - 1);
    if (y + 1 < H) {
        const int e = disp[i + W];
        if (speckle_joined(d, e, invalid, max_diff)) {
            const bool implied = left && speckle_joined(disp[i + W - 1], e, invalid, max_diff) && speckle_joined(disp[i - 1], disp[i + W - 1], invalid, max_diff);
            if (!implied) uf_union(labels, i, i + W);
        }
    }
}

// one atomicAdd per distinct root of a wavefront, not per pixel: a map that is one large component would otherwise send every
// pixel's increment to the same address.  Whole blocks run: the ballots need every lane.
__global__ __launch_bounds__(256) void speckle_count_kernel(int* __restrict__ labels, int* __restrict__ counts, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
    int root = -1;
    if (i < n && labels[i] >= 0) {
        root = uf_find(labels, i);
        labels[i] = root;   // an ancestor, like every store of uf_find
    }
    unsigned long long todo = __ballot(root >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int r0 = __shfl(root, leader);
        const unsigned long long same = __ballot(root == r0);
        if (lane == leader) atomicAdd(&counts[r0], __popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256) void speckle_clear_kernel(int16_t* __restrict__ disp, int* __restrict__ labels, const int* __restrict__ counts, int n,
                                                            int invalid, int max_size) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || labels[i] < 0) return;
    if (counts[uf_find(labels, i)] <= max_size) disp[i] = (int16_t)invalid;
}

// n = images * H * W pixels of `disp`; workspace: speckle_layout(n)
static int speckle_launch(int16_t* disp, int images, int H, int W, int invalid, int max_size, int max_diff, void* workspace, hipStream_t s) {
    const int n = images * H * W, blocks = (n + 255) / 256;
    const SpeckleWs ws = speckle_layout(workspace, n);
    int *labels = ws.labels, *counts = ws.counts;
    const double px = (double)n;
    {
        ProfScope prof("speckle_init_kernel", px, 10.0 * px, s);
        hipLaunchKernelGGL(speckle_init_kernel, dim3(blocks), dim3(256), 0, s, disp, labels, counts, n, W, invalid, max_diff);
    }
    {
        ProfScope prof("speckle_merge_kernel", 8.0 * px, 14.0 * px, s);
        hipLaunchKernelGGL(speckle_merge_kernel, dim3(blocks), dim3(256), 0, s, disp, labels, n, H, W, invalid, max_diff);
    }
    {
        ProfScope prof("speckle_count_kernel", 2.0 * px, 12.0 * px, s);
        hipLaunchKernelGGL(speckle_count_kernel, dim3(blocks), dim3(256), 0, s, labels, counts, n);
    }
    {
        ProfScope prof("speckle_clear_kernel", px, 10.0 * px, s);
        hipLaunchKernelGGL(speckle_clear_kernel, dim3(blocks), dim3(256), 0, s, disp, labels, counts, n, invalid, max_size);
    }
    return check_launch("speckle kernels");
}

// ---------------------------------------------------------------- host side
struct StereoPlan {
    int Wv, r, TY, group;
    size_t volume;   // elements of one image's cost volume (and of S)
    size_t bytes;    // stereo_layout of `group` images
};

// the checks that need no pointer; 0 = fine
static int stereo_check(const char* who, int B, int H, int W, int C, int min_disp, int num_disp, int block, StereoPlan* plan) {
    if (B < 1 || H < 1 || W < 1) return fail(WMD_ERR_BAD_SHAPE, "%s: B=%d H=%d W=%d", who, B, H, W);
    if (C != 1 && C != 3) return fail(WMD_ERR_BAD_ARG, "%s: C=%d channels, 1 or 3 expected", who, C);
    if (min_disp < 0) return fail(WMD_ERR_BAD_ARG, "%s: minDisparity=%d is negative", who, min_disp);
    if (num_disp < 16 || num_disp > 256 || num_disp % 16) return fail(WMD_ERR_BAD_ARG, "%s: numDisparities=%d, a multiple of 16 in 16..256 expected", who, num_disp);
    if (block < 1) return fail(WMD_ERR_BAD_ARG, "%s: blockSize=%d", who, block);
    if (W <= min_disp + num_disp) return fail(WMD_ERR_BAD_SHAPE, "%s: W=%d leaves no column right of minDisparity + numDisparities = %d", who, W, min_disp + num_disp);
    if (W > 65535 || B > 65535 || H > 65535) return fail(WMD_ERR_UNSUPPORTED, "%s: B, H and W up to 65535 (got %d, %d, %d)", who, B, H, W);
    StereoPlan p;
    p.Wv = W - min_disp - num_disp, p.r = block / 2;
    const double vol = (double)H * p.Wv * num_disp;
    if (vol > 2147483647.0 || (double)B * H * W > 2147483647.0) return fail(WMD_ERR_UNSUPPORTED, "%s: more than 2^31 elements in one cost volume or in the maps", who);
    p.TY = 0;
    for (int ty = 4; ty >= 1 && !p.TY; ty >>= 1)
        if (cost_tile(ty, p.r, C, num_disp).bytes <= kCostLdsMax) p.TY = ty;
    if (!p.TY) return fail(WMD_ERR_UNSUPPORTED, "%s: a blockSize=%d window over %d disparities does not fit the cost kernel's LDS tile", who, block, num_disp);
    p.volume = (size_t)vol;
    p.group = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, kStereoGroupCap / stereo_layout(nullptr, 1, H, W, C, p.volume).bytes));
    p.bytes = stereo_layout(nullptr, p.group, H, W, C, p.volume).bytes;
    if (plan) *plan = p;
    return WMD_OK;
}

template <int NR>
static void path_launch(const uint16_t* cost, uint16_t* S, int G, int H, int Wv, int D, int sx, int sy, int P1, int P2, int first, size_t stride, hipStream_t s) {
    const int lines = sy == 0 ? H : (sx == 0 ? Wv : Wv + H - 1);
    hipLaunchKernelGGL(stereo_path_kernel<NR>, dim3((lines + 3) / 4, 1, G), dim3(256), 0, s, cost, S, H, Wv, D, sx, sy, P1, P2, first, stride);
}

template <int NR>
static void winner_launch(const uint16_t* S, int16_t* first_map, unsigned* keys, int G, int H, int W, int minD, int D, int uniq, size_t stride, hipStream_t s) {
    const int pix = H * (W - minD - D);
    hipLaunchKernelGGL(stereo_winner_kernel<NR>, dim3((pix + 3) / 4, 1, G), dim3(256), 0, s, S, first_map, keys, H, W, minD, D, uniq, stride);
}

}  // namespace wmd

using namespace wmd;

extern "C" size_t wmd_stereo_sgbm_workspace_bytes(int B, int H, int W, int C, int min_disp, int num_disp, int block) {
    StereoPlan p;
    if (stereo_check("wmd_stereo_sgbm_workspace_bytes", B, H, W, C, min_disp, num_disp, block, &p) != WMD_OK) return 0;
    return p.bytes;
}

extern "C" size_t wmd_stereo_filter_speckles_workspace_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (double)B * H * W > 2147483647.0) return 0;
    return speckle_layout(nullptr, (size_t)B * H * W).bytes;
}

extern "C" int wmd_stereo_filter_speckles(short* disp, int B, int H, int W, int invalid, int max_size, int max_diff, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    const char* who = "wmd_stereo_filter_speckles";
    if (!disp || !workspace) return fail(WMD_ERR_BAD_ARG, "%s: null pointer (disp or workspace)", who);
    if (B < 1 || H < 1 || W < 1) return fail(WMD_ERR_BAD_SHAPE, "%s: B=%d H=%d W=%d", who, B, H, W);
    if (max_size < 0 || max_diff < 0 || invalid < -32768 || invalid > 32767)
        return fail(WMD_ERR_BAD_ARG, "%s: max_size=%d max_diff=%d invalid=%d", who, max_size, max_diff, invalid);
    const size_t need = wmd_stereo_filter_speckles_workspace_bytes(B, H, W);
    if (!need) return fail(WMD_ERR_UNSUPPORTED, "%s: more than 2^31 pixels", who);
    if (int st = check_workspace(who, workspace, workspace_bytes, need, 4, WMD_ERR_WORKSPACE)) return st;
    return speckle_launch((int16_t*)disp, B, H, W, invalid, max_size, max_diff, workspace, (hipStream_t)stream);
}

extern "C" int wmd_stereo_sgbm(const unsigned char* left, const unsigned char* right, const unsigned char* reverse, short* disp,
                               unsigned short* cost_out, unsigned short* S_out, int B, int H, int W, int C, int min_disp, int num_disp,
                               int block, int P1, int P2, int cap, int uniq, int speckle_win, int speckle_range, int disp12,
                               int directions, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "wmd_stereo_sgbm";
    if (!left || !right || !disp || !workspace) return fail(WMD_ERR_BAD_ARG, "%s: null pointer (left, right, disp or workspace)", who);
    StereoPlan p;
    const int st = stereo_check(who, B, H, W, C, min_disp, num_disp, block, &p);
    if (st != WMD_OK) return st;
    if (P1 < 0 || P1 > P2) return fail(WMD_ERR_BAD_ARG, "%s: P1=%d P2=%d, 0 <= P1 <= P2 expected", who, P1, P2);
    if (directions != 5 && directions != 8) return fail(WMD_ERR_BAD_ARG, "%s: directions=%d, 5 or 8 expected", who, directions);
    if (uniq < 0 || uniq > 100 || speckle_win < 0 || speckle_range < 0 || cap < 0)
        return fail(WMD_ERR_BAD_ARG, "%s: uniquenessRatio=%d speckleWindowSize=%d speckleRange=%d preFilterCap=%d", who, uniq, speckle_win, speckle_range, cap);
    if (cap > 127) return fail(WMD_ERR_UNSUPPORTED, "%s: preFilterCap=%d, the prefiltered signal is stored in 8 bits (cap <= 127)", who, cap);
    const int win = 2 * p.r + 1;
    const double bound = (double)directions * ((double)win * win * C * (2 * cap + 63) + P2);
    if (bound > 65535.0) return fail(WMD_ERR_UNSUPPORTED, "%s: S can reach %.0f with these settings, the volumes hold 16 bits", who, bound);
    if (speckle_range > 2047) return fail(WMD_ERR_UNSUPPORTED, "%s: speckleRange=%d", who, speckle_range);
    if (int st2 = check_workspace(who, workspace, workspace_bytes, p.bytes, 256, WMD_ERR_WORKSPACE)) return st2;

    hipStream_t s = (hipStream_t)stream;
    const int D = num_disp, Wv = p.Wv, NR = (D + 63) / 64, tol = disp12 > 0 ? disp12 : 1, invalid = (min_disp - 1) * 16;
    const StereoWs ws = stereo_layout(workspace, p.group, H, W, C, p.volume);
    const size_t vol_stride = stereo_stride<uint16_t>(p.volume);
    static const int steps[8][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}, {-1, -1}, {0, -1}, {1, -1}};   // minus the predecessor offsets
    const CostTile tile = cost_tile(p.TY, p.r, C, D);

    for (int b0 = 0; b0 < B; b0 += p.group) {
        const int G = std::min(p.group, B - b0);
        // a caller's volume is [B][H][Wv][D] dense; the workspace's images sit vol_stride apart
        uint16_t* cost = cost_out ? cost_out + (size_t)b0 * p.volume : ws.cost;
        uint16_t* S = S_out ? S_out + (size_t)b0 * p.volume : ws.S;
        const size_t cstride = cost_out ? p.volume : vol_stride, sstride = S_out ? p.volume : vol_stride;
        const double px = (double)G * H * W, vol = (double)G * p.volume;
        {
            ProfScope prof("stereo_prep_kernel", 60.0 * px * C * 2, px * C * 2 * (9.0 + 8.0), s);
            hipLaunchKernelGGL(stereo_prep_kernel, dim3((W * C + 255) / 256, H, 2 * G), dim3(256), 0, s, left, right, reverse, ws.prep, b0, H, W, C, cap);
        }
        {
            ProfScope prof("stereo_cost_kernel", vol * (20.0 * C * tile.rows * tile.LW / (p.TY * kCostTX) + win * win), 2.0 * vol + 16.0 * px * C, s);
            hipLaunchKernelGGL(stereo_cost_kernel, dim3((Wv + kCostTX - 1) / kCostTX, (H + p.TY - 1) / p.TY, G), dim3(kCostThreads), tile.bytes, s, ws.prep, cost,
                               H, W, C, min_disp, D, p.r, p.TY, cstride);
        }
        for (int k = 0; k < directions; ++k) {
            const int sx = steps[k][0], sy = steps[k][1], first = k == 0;
            ProfScope prof("stereo_path_kernel", 12.0 * vol, (first ? 4.0 : 6.0) * vol, s);
            if (cstride != sstride) {
                // one stride serves both volumes in the kernel: a caller's volume on one side only goes image by image
                for (int g = 0; g < G; ++g) {
                    const uint16_t* cg = cost + (size_t)g * cstride;
                    uint16_t* sg = S + (size_t)g * sstride;
                    switch (NR) {
                        case 1: path_launch<1>(cg, sg, 1, H, Wv, D, sx, sy, P1, P2, first, 0, s); break;
                        case 2: path_launch<2>(cg, sg, 1, H, Wv, D, sx, sy, P1, P2, first, 0, s); break;
                        case 3: path_launch<3>(cg, sg, 1, H, Wv, D, sx, sy, P1, P2, first, 0, s); break;
                        default: path_launch<4>(cg, sg, 1, H, Wv, D, sx, sy, P1, P2, first, 0, s); break;
                    }
                }
            } else {
                switch (NR) {
                    case 1: path_launch<1>(cost, S, G, H, Wv, D, sx, sy, P1, P2, first, cstride, s); break;
                    case 2: path_launch<2>(cost, S, G, H, Wv, D, sx, sy, P1, P2, first, cstride, s); break;
                    case 3: path_launch<3>(cost, S, G, H, Wv, D, sx, sy, P1, P2, first, cstride, s); break;
                    default: path_launch<4>(cost, S, G, H, Wv, D, sx, sy, P1, P2, first, cstride, s); break;
                }
            }
        }
        if (hipMemsetAsync(ws.keys, 0xFF, (size_t)G * H * W * sizeof(unsigned), s) != hipSuccess) return check_launch("stereo keys memset");
        {
            ProfScope prof("stereo_winner_kernel", 6.0 * vol, 2.0 * vol + 10.0 * px, s);
            switch (NR) {
                case 1: winner_launch<1>(S, ws.first_map, ws.keys, G, H, W, min_disp, D, uniq, sstride, s); break;
                case 2: winner_launch<2>(S, ws.first_map, ws.keys, G, H, W, min_disp, D, uniq, sstride, s); break;
                case 3: winner_launch<3>(S, ws.first_map, ws.keys, G, H, W, min_disp, D, uniq, sstride, s); break;
                default: winner_launch<4>(S, ws.first_map, ws.keys, G, H, W, min_disp, D, uniq, sstride, s); break;
            }
        }
        {
            ProfScope prof("stereo_finish_kernel", 10.0 * px, 12.0 * px, s);
            hipLaunchKernelGGL(stereo_finish_kernel, dim3((W + 255) / 256, H, G), dim3(256), 0, s, ws.first_map, ws.keys, reverse, (int16_t*)disp, b0, H, W, min_disp,
                               D, tol);
        }
        const int st2 = check_launch("stereo kernels");
        if (st2 != WMD_OK) return st2;
        if (speckle_win > 0) {
            const int st3 = speckle_launch((int16_t*)disp + (size_t)b0 * H * W, G, H, W, invalid, speckle_win, 16 * speckle_range, ws.speckle, s);
            if (st3 != WMD_OK) return st3;
        }
    }
    return WMD_OK;
}
