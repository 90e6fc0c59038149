// Device arithmetic shared by the photometric kernels (wmd_photo.hip) and the depth-hint fusion (wmd_hints.hip): the
// ReflectionPad2d(1) index, the SSIM window statistics and value, and the BackprojectDepth -> Project3D -> grid_sample
// geometry.  One definition, so that a hint is scored by exactly the arithmetic the trainer's loss uses.
#pragma once
#include "wmd_internal.h"

namespace wmd {

__device__ __forceinline__ int refl1(int g, int n) {   // ReflectionPad2d(1) source index of padded coordinate g in [-1, n]
    return g < 0 ? -g : (g >= n ? 2 * n - 2 - g : g);
}

// ------------------------------------------------------------------------------------------------
// SSIM / reprojection loss
// ------------------------------------------------------------------------------------------------
struct SsimStats {
    float mx, my, ex2, ey2, exy;
};

__device__ __forceinline__ SsimStats ssim_window(const float* __restrict__ xp, const float* __restrict__ yp, int y, int x, int H, int W) {
    float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int ry = refl1(y + dy, H) * W;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int rx = refl1(x + dx, W);
            const float a = xp[ry + rx], b = yp[ry + rx];
            sx += a;
            sy += b;
            sxx += a * a;
            syy += b * b;
            sxy += a * b;
        }
    }
    const float inv9 = 1.f / 9.f;
    return SsimStats{sx * inv9, sy * inv9, sxx * inv9, syy * inv9, sxy * inv9};
}

constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

__device__ __forceinline__ float ssim_value(const SsimStats& s, float* n1o = nullptr, float* n2o = nullptr, float* d1o = nullptr,
                                            float* d2o = nullptr) {
    const float sig_x = s.ex2 - s.mx * s.mx, sig_y = s.ey2 - s.my * s.my, sig_xy = s.exy - s.mx * s.my;
    const float n1 = 2.f * s.mx * s.my + kC1, n2 = 2.f * sig_xy + kC2;
    const float d1 = s.mx * s.mx + s.my * s.my + kC1, d2 = sig_x + sig_y + kC2;
    if (n1o) *n1o = n1, *n2o = n2, *d1o = d1, *d2o = d2;
    return (n1 * n2) / (d1 * d2);
}

// ------------------------------------------------------------------------------------------------
// warp: BackprojectDepth -> Project3D -> grid_sample(bilinear, padding_mode="border", align_corners=False)
// ------------------------------------------------------------------------------------------------
struct WarpGeom {       // everything about one target pixel that forward and backward share
    float rx, ry, rz;   // inv_K[:3,:3] * (x, y, 1)
    float X, Y, Z;      // depth * r
    float u, v, w;      // P * (X, Y, Z, 1)
    float ix, iy;       // clipped source coordinates
    float mx, my;       // clip gradient multipliers (0 where the border clamp is active)
};

__device__ __forceinline__ void warp_P(const float* __restrict__ K, const float* __restrict__ T, float* P) {   // (K T)[:3,:]
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += K[i * 4 + k] * T[k * 4 + j];
            P[i * 4 + j] = s;
        }
}

__device__ __forceinline__ float clip_coord(float in, int size, float* mult) {   // ATen clip_coordinates_set_grad
    // written so that a NaN coordinate (depth 0 x inf, a degenerate pose) lands on 0 with zero gradient instead of
    // slipping through both comparisons and being cast to an int: ATen never indexes with a NaN either
    const float mx = (float)(size - 1);
    const bool inside = in > 0.f && in < mx;          // false for NaN
    *mult = inside ? 1.f : 0.f;
    return inside ? in : (in >= mx ? mx : 0.f);       // NaN -> 0
}

__device__ __forceinline__ WarpGeom warp_geom(float depth, int x, int y, const float* __restrict__ iK, const float* P, int H, int W,
                                              int Hs, int Ws, float eps) {
    WarpGeom g;
    g.rx = iK[0] * x + iK[1] * y + iK[2];
    g.ry = iK[4] * x + iK[5] * y + iK[6];
    g.rz = iK[8] * x + iK[9] * y + iK[10];
    g.X = depth * g.rx;
    g.Y = depth * g.ry;
    g.Z = depth * g.rz;
    g.u = P[0] * g.X + P[1] * g.Y + P[2] * g.Z + P[3];
    g.v = P[4] * g.X + P[5] * g.Y + P[6] * g.Z + P[7];
    g.w = P[8] * g.X + P[9] * g.Y + P[10] * g.Z + P[11];
    const float den = g.w + eps;
    float gx = (g.u / den) / (float)(W - 1), gy = (g.v / den) / (float)(H - 1);   // Project3D: /= (width - 1), (x - 0.5) * 2
    gx = (gx - 0.5f) * 2.f;
    gy = (gy - 0.5f) * 2.f;
    const float ux = ((gx + 1.f) * Ws - 1.f) * 0.5f, uy = ((gy + 1.f) * Hs - 1.f) * 0.5f;   // grid_sampler_unnormalize
    g.ix = clip_coord(ux, Ws, &g.mx);
    g.iy = clip_coord(uy, Hs, &g.my);
    return g;
}

}  // namespace wmd
