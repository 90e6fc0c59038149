// Depth-hint fusion (KITTI/precompute_depth_hints.py:243-249 with the disparity conversion of :149): M candidate depth maps
// of one stereo pair -> per pixel the depth of the candidate whose reprojection of the other view matches the base image best
// (0.85 SSIM + 0.15 L1, the trainer's compute_reprojection_loss).  The reference expands both images M-fold and runs
// BackprojectDepth, Project3D, grid_sample, SSIM, argmin and gather; here it is one launch that reads every candidate plane
// and the base image once and writes two planes (plus the M loss planes on request).  The candidates are the caller's, from
// any matcher; wmd_stereo.hip is the library's.
//
// hints_fuse_kernel: a block of 256 threads (4 wavefronts) owns a 64 x 8 output tile; wavefront q owns rows 2q and 2q + 1,
// lane x column x.  Per candidate the block warps the tile plus its one-pixel ReflectionPad2d ring (66 x 10 positions, each
// with its own candidate depth, the ring at the reflected pixel) into LDS -- up to three colour planes and the depth plane --
// and after one barrier every thread reads a 3 x 4 window per channel and scores its two pixels.  The two LDS buffers
// alternate, so the fill of candidate m + 1 can overtake the reads of candidate m and one barrier per candidate is enough:
// buffer m & 1 is written again only by threads that have passed barrier m + 1, which every thread reaches after its reads
// of candidate m.  The base image's 3 x 4 windows, their sums and the running minimum stay in registers for all M
// candidates.  LDS rows are read by 64 consecutive lanes at consecutive dwords: no bank conflicts.
#include <algorithm>
#include "wmd_internal.h"
#include "wmd_photo_common.h"

namespace wmd {

constexpr int kHintTW = 64, kHintTH = 8, kHintRows = 2;           // tile; rows per thread
constexpr int kHintHW = kHintTW + 2, kHintHH = kHintTH + 2;       // tile + ring
constexpr int kHintHalo = kHintHW * kHintHH;                      // 660 positions
constexpr int kHintDepthPlane = 3;                                // LDS planes 0..2: colour, 3: the depth that was warped
constexpr int kHintThreads = kHintTW * (kHintTH / kHintRows);     // 256

__device__ __forceinline__ float hint_depth(float v, int is_disparity, float fbl) {
    return is_disparity ? fbl / (v + 1e-7f) * (v > 0.f ? 1.f : 0.f) : v;   // precompute_depth_hints.py:149
}

// 168 VGPRs without spilling: three blocks per CU, so the 640 blocks of one 320 x 1024 image are resident at once (768 slots)
__global__ __launch_bounds__(kHintThreads, 3) void hints_fuse_kernel(const float* __restrict__ cand, int is_disparity, float fbl,
                                                                  const float* __restrict__ base, const float* __restrict__ lookup,
                                                                  const float* __restrict__ K, const float* __restrict__ iK,
                                                                  const float* __restrict__ T, float* __restrict__ best_depth,
                                                                  int* __restrict__ best_index, float* __restrict__ losses, int M,
                                                                  int C, int H, int W, float eps, float w_ssim, float w_l1) {
    __shared__ float tile[2][4][kHintHalo];
    const int b = blockIdx.z, x0 = blockIdx.x * kHintTW, y0 = blockIdx.y * kHintTH;
    const int tx = threadIdx.x & (kHintTW - 1), r0 = (threadIdx.x >> 6) * kHintRows;
    const size_t plane = (size_t)H * W;
    float P[12];
    warp_P(K + b * 16, T + b * 16, P);
    const float* iKb = iK + b * 16;
    const float inv9 = 1.f / 9.f, invC = 1.f / (float)C;

    // the base image: 3 x 4 window per channel and the window sums of the two pixels, once for all candidates.  Threads of
    // a ragged tile that lie outside the image read clamped coordinates and write nothing.
    float bw[3][kHintRows + 2][3], bmean[3][kHintRows], bsq[3][kHintRows];
    const int xc = min(x0 + tx, W - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c < C) {
            const float* bp = base + ((size_t)b * C + c) * plane;
#pragma unroll
            for (int j = 0; j < kHintRows + 2; ++j) {
                const int ry = refl1(min(y0 + r0 - 1 + j, H), H);
#pragma unroll
                for (int i = 0; i < 3; ++i) bw[c][j][i] = bp[(size_t)ry * W + refl1(xc - 1 + i, W)];
            }
#pragma unroll
            for (int p = 0; p < kHintRows; ++p) {
                float s = 0.f, ss = 0.f;
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float v = bw[c][p + j][i];
                        s += v;
                        ss += v * v;
                    }
                bmean[c][p] = s * inv9;
                bsq[c][p] = ss * inv9;
            }
        }
    }

    float best[kHintRows], bdep[kHintRows];
    int bidx[kHintRows];
#pragma unroll
    for (int p = 0; p < kHintRows; ++p) best[p] = 0.f, bdep[p] = 0.f, bidx[p] = 0;

    for (int m = 0; m < M; ++m) {
        float(*buf)[kHintHalo] = tile[m & 1];
        const float* cp = cand + ((size_t)b * M + m) * plane;
        for (int i = threadIdx.x; i < kHintHalo; i += kHintThreads) {
            const int hy = i / kHintHW, hx = i - hy * kHintHW;
            const int gy = refl1(min(y0 - 1 + hy, H), H), gx = refl1(min(x0 - 1 + hx, W), W);
            const float depth = hint_depth(cp[(size_t)gy * W + gx], is_disparity, fbl);
            const WarpGeom g = warp_geom(depth, gx, gy, iKb, P, H, W, H, W, eps);
            // the bilinear sample of warp_fwd_kernel (wmd_photo.hip), expression for expression
            const float fx0 = floorf(g.ix), fy0 = floorf(g.iy);
            const int sx0 = (int)fx0, sy0 = (int)fy0, sx1 = sx0 + 1, sy1 = sy0 + 1;
            const float ax = g.ix - fx0, ay = g.iy - fy0;
            const bool in_x1 = sx1 < W, in_y1 = sy1 < H;   // sx0, sy0 are inside after the clip
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c < C) {
                    const float* s = lookup + ((size_t)b * C + c) * plane;
                    const float v00 = s[(size_t)sy0 * W + sx0], v01 = in_x1 ? s[(size_t)sy0 * W + sx1] : 0.f;
                    const float v10 = in_y1 ? s[(size_t)sy1 * W + sx0] : 0.f, v11 = (in_x1 && in_y1) ? s[(size_t)sy1 * W + sx1] : 0.f;
                    buf[c][i] = v00 * (1.f - ax) * (1.f - ay) + v01 * ax * (1.f - ay) + v10 * (1.f - ax) * ay + v11 * ax * ay;
                }
            }
            buf[kHintDepthPlane][i] = depth;
        }
        __syncthreads();

        float ssim_sum[kHintRows], l1_sum[kHintRows];
#pragma unroll
        for (int p = 0; p < kHintRows; ++p) ssim_sum[p] = 0.f, l1_sum[p] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < C) {
                float w[kHintRows + 2][3];
#pragma unroll
                for (int j = 0; j < kHintRows + 2; ++j)
#pragma unroll
                    for (int i = 0; i < 3; ++i) w[j][i] = buf[c][(r0 + j) * kHintHW + tx + i];
#pragma unroll
                for (int p = 0; p < kHintRows; ++p) {
                    float sx = 0.f, sxx = 0.f, sxy = 0.f;   // x = the warped view (pred), y = the base image (target)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const float a = w[p + j][i];
                            sx += a;
                            sxx += a * a;
                            sxy += a * bw[c][p + j][i];
                        }
                    const float s = ssim_value(SsimStats{sx * inv9, bmean[c][p], sxx * inv9, bsq[c][p], sxy * inv9});
                    ssim_sum[p] += fminf(fmaxf((1.f - s) * 0.5f, 0.f), 1.f);
                    l1_sum[p] += fabsf(bw[c][p + 1][1] - w[p + 1][1]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < kHintRows; ++p) {
            const float loss = w_ssim * (ssim_sum[p] * invC) + w_l1 * (l1_sum[p] * invC);
            if (m == 0 || loss < best[p]) {   // strict <: the lowest index wins among equal losses, like argmin on the CPU
                best[p] = loss;
                bidx[p] = m;
                bdep[p] = buf[kHintDepthPlane][(r0 + p + 1) * kHintHW + tx + 1];
            }
            const int y = y0 + r0 + p, x = x0 + tx;
            if (losses && y < H && x < W) losses[((size_t)b * M + m) * plane + (size_t)y * W + x] = loss;
        }
    }
#pragma unroll
    for (int p = 0; p < kHintRows; ++p) {
        const int y = y0 + r0 + p, x = x0 + tx;
        if (y < H && x < W) {
            best_depth[(size_t)b * plane + (size_t)y * W + x] = bdep[p];
            best_index[(size_t)b * plane + (size_t)y * W + x] = bidx[p];
        }
    }
}

}  // namespace wmd

using namespace wmd;

extern "C" size_t wmd_depth_hints_workspace_floats(int B, int M, int H, int W) {
    (void)B, (void)M, (void)H, (void)W;
    return 0;   // the tile lives in LDS, the running minimum in registers: nothing is staged in device memory
}

extern "C" int wmd_depth_hints_fuse(const float* cand, int cand_is_disparity, float focal_times_baseline, const float* base,
                                    const float* lookup, const float* K, const float* inv_K, const float* T, float* best_depth,
                                    int* best_index, float* losses, int B, int M, int C, int H, int W, float eps, float w_ssim,
                                    float w_l1, float* workspace, size_t workspace_floats, void* stream) {
    const char* who = "wmd_depth_hints_fuse";
    if (!cand || !base || !lookup || !K || !inv_K || !T || !best_depth || !best_index) return fail(WMD_ERR_BAD_ARG, "%s: null tensor pointer", who);
    if (B <= 0 || M < 1 || C < 1 || H < 2 || W < 2)
        return fail(WMD_ERR_BAD_SHAPE, "%s: B=%d M=%d C=%d H=%d W=%d (M, C >= 1; reflection padding needs H, W >= 2)", who, B, M, C, H, W);
    if (M > WMD_DEPTH_HINTS_MAX_CANDIDATES) return fail(WMD_ERR_UNSUPPORTED, "%s: M=%d candidates, at most %d", who, M, WMD_DEPTH_HINTS_MAX_CANDIDATES);
    if (C > 3) return fail(WMD_ERR_UNSUPPORTED, "%s: C=%d channels, at most 3", who, C);
    if (B > 65535 || H > 65535 * kHintTH || (double)B * std::max(M, C) * H * W > 2147483647.0)
        return fail(WMD_ERR_UNSUPPORTED, "%s: more than 2^31 elements, B > 65535 or H > %d", who, 65535 * kHintTH);
    if (int st = check_workspace_floats(who, workspace, workspace_floats, wmd_depth_hints_workspace_floats(B, M, H, W))) return st;
    hipStream_t s = (hipStream_t)stream;
    const double n = (double)B * H * W;
    ProfScope prof("hints_fuse_kernel", n * M * (80.0 + 75.0 * C), 4.0 * n * (M * (losses ? 2.0 : 1.0) + C + 2.0), s);
    hipLaunchKernelGGL(hints_fuse_kernel, dim3((W + kHintTW - 1) / kHintTW, (H + kHintTH - 1) / kHintTH, B), dim3(kHintThreads), 0, s, cand,
                       cand_is_disparity, focal_times_baseline, base, lookup, K, inv_K, T, best_depth, best_index, losses, M, C, H, W, eps,
                       w_ssim, w_l1);
    return check_launch("hints_fuse_kernel");
}
