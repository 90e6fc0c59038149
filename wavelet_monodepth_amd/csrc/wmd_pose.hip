// The pose path between the pose trunk and the warp (include/wmd.h, "Pose networks"):
//   wmd_pose_transform_fwd / _bwd   (axis-angle, translation) -> 4x4 camera transform, KITTI/layers.py:42-117
//   wmd_pose_head_fwd / _bwd        1x1 convolution + spatial mean + scale (the tail of PoseDecoder / PoseCNN), with the
//                                   transform of every predicted frame from the same launch
// The work is a few thousand FLOPs behind ~120 KB of reads per image: what counts is the number of launches (one forward,
// two backward) and that every sum runs in a fixed order (no atomics), so that two runs give the same bits.
#include "wmd_internal.h"

namespace wmd {
namespace {

constexpr int kMaxFrames = 4;               // F: 6 F <= 24 outputs per image
constexpr int kMaxOut = 6 * kMaxFrames;
constexpr int kHeadThreads = 1024;          // forward: 16 waves per image
constexpr int kDxChannels = 32;             // backward: channels per dx block
constexpr float kAxisEps = 1e-7f;           // axis = v / (|v| + 1e-7), not renormalised

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// R = cos(angle) I + (1 - cos(angle)) a a^T + sin(angle) [a]x, with 1 - cos as 2 sin^2(angle / 2) (no cancellation at small
// angles).  At v = 0: a = 0, sin = 0, cos = 1, so R is the identity bit for bit.
struct Rot {
    float ax, ay, az, s, c, C, inv;   // inv = 1 / (angle + eps)
    float angle;
};

__device__ __forceinline__ Rot rot_terms(float vx, float vy, float vz) {
    Rot r;
    r.angle = sqrtf(vx * vx + vy * vy + vz * vz);
    r.inv = 1.f / (r.angle + kAxisEps);
    r.ax = vx * r.inv;
    r.ay = vy * r.inv;
    r.az = vz * r.inv;
    sincosf(r.angle, &r.s, &r.c);
    const float sh = sinf(0.5f * r.angle);
    r.C = 2.f * sh * sh;
    return r;
}

__device__ __forceinline__ void rot_matrix(const Rot& r, float R[3][3]) {
    const float xC = r.ax * r.C, yC = r.ay * r.C, zC = r.az * r.C;
    const float xs = r.ax * r.s, ys = r.ay * r.s, zs = r.az * r.s;
    const float xyC = r.ax * yC, yzC = r.ay * zC, zxC = r.az * xC;
    R[0][0] = r.ax * xC + r.c;
    R[0][1] = xyC - zs;
    R[0][2] = zxC + ys;
    R[1][0] = xyC + zs;
    R[1][1] = r.ay * yC + r.c;
    R[1][2] = yzC - xs;
    R[2][0] = zxC - ys;
    R[2][1] = yzC + xs;
    R[2][2] = r.az * zC + r.c;
}

// v, t: 3 floats each; T: 16 floats, row-major.  Not inverted: [[R, t], [0, 1]]; inverted: [[R^T, -R^T t], [0, 1]].
__device__ __forceinline__ void pose_transform(const float* v, const float* t, bool invert, float* T) {
    float R[3][3];
    rot_matrix(rot_terms(v[0], v[1], v[2]), R);
    const float tx = t[0], ty = t[1], tz = t[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[4 * i + j] = invert ? R[j][i] : R[i][j];
        T[4 * i + 3] = invert ? -(R[0][i] * tx + R[1][i] * ty + R[2][i] * tz) : (i == 0 ? tx : (i == 1 ? ty : tz));
    }
    T[12] = 0.f;
    T[13] = 0.f;
    T[14] = 0.f;
    T[15] = 1.f;
}

// The derivative of pose_transform as autograd writes it for the expression above, the 1e-7 included; G: 16 floats (the bottom
// row is constant and ignored).  At v = 0 every term of dv carries a factor a = 0 or sin = 0: dv is exactly 0.
__device__ __forceinline__ void pose_transform_bwd(const float* v, const float* t, bool invert, const float* G, float* dv, float* dt) {
    const Rot r = rot_terms(v[0], v[1], v[2]);
    float dR[3][3];
    if (!invert) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) dR[i][j] = G[4 * i + j];
            dt[i] = G[4 * i + 3];
        }
    } else {
        float R[3][3];
        rot_matrix(r, R);
        const float p0 = G[3], p1 = G[7], p2 = G[11];   // the gradient of the column -R^T t
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float ti = t[i];
            dR[i][0] = G[4 * 0 + i] - ti * p0;
            dR[i][1] = G[4 * 1 + i] - ti * p1;
            dR[i][2] = G[4 * 2 + i] - ti * p2;
            dt[i] = -(R[i][0] * p0 + R[i][1] * p1 + R[i][2] * p2);
        }
    }
    const float a[3] = {r.ax, r.ay, r.az};
    const float dc = dR[0][0] + dR[1][1] + dR[2][2];
    float dC = 0.f, da[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float sym = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            dC += dR[i][j] * a[i] * a[j];
            sym += (dR[i][j] + dR[j][i]) * a[j];
        }
        da[i] = r.C * sym;
    }
    const float kx = dR[2][1] - dR[1][2], ky = dR[0][2] - dR[2][0], kz = dR[1][0] - dR[0][1];   // the skew part of dR
    const float ds = a[0] * kx + a[1] * ky + a[2] * kz;
    da[0] += r.s * kx;
    da[1] += r.s * ky;
    da[2] += r.s * kz;
    // angle enters through cos, 1 - cos, sin and the denominator of a = v / (angle + eps)
    const float dangle = r.s * (dC - dc) + r.c * ds - (da[0] * v[0] + da[1] * v[1] + da[2] * v[2]) * r.inv * r.inv;
    const float unit = r.angle > 0.f ? 1.f / r.angle : 0.f;   // d|v| / dv = v / |v|, 0 at v = 0
#pragma unroll
    for (int i = 0; i < 3; ++i) dv[i] = da[i] * r.inv + dangle * v[i] * unit;
}

__global__ void __launch_bounds__(256) pose_transform_fwd_kernel(const float* __restrict__ axisangle, const float* __restrict__ translation,
                                                                 float* __restrict__ T, int N, int invert) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float v[3], t[3], M[16];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = axisangle[3 * (size_t)n + k];
        t[k] = translation[3 * (size_t)n + k];
    }
    pose_transform(v, t, invert != 0, M);
#pragma unroll
    for (int k = 0; k < 16; ++k) T[16 * (size_t)n + k] = M[k];
}

__global__ void __launch_bounds__(256) pose_transform_bwd_kernel(const float* __restrict__ axisangle, const float* __restrict__ translation,
                                                                 const float* __restrict__ dT, float* __restrict__ d_axisangle,
                                                                 float* __restrict__ d_translation, int N, int invert) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float v[3], t[3], G[16], dv[3], dt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = axisangle[3 * (size_t)n + k];
        t[k] = translation[3 * (size_t)n + k];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) G[k] = dT[16 * (size_t)n + k];
    pose_transform_bwd(v, t, invert != 0, G, dv, dt);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d_axisangle[3 * (size_t)n + k] = dv[k];
        d_translation[3 * (size_t)n + k] = dt[k];
    }
}

// One block per image.  Phase 1: a wave per channel sums its H W values (float4 loads when every row is 16-byte aligned, lane
// partials then a butterfly: a fixed order) -> means[b, c], kept in LDS.  Phase 2: a wave per output o: scale * (bias[o] +
// w[o, :] . mean).  Phase 3: a lane per frame builds T.
__global__ void __launch_bounds__(kHeadThreads) pose_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, float* __restrict__ params,
                                                                     float* __restrict__ T, float* __restrict__ means, int C, int HW,
                                                                     int F, int invert_mask, float scale, int vec4) {
    extern __shared__ float smem[];   // C means, then 6 F parameters
    float* mean_s = smem;
    float* par_s = smem + C;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = kHeadThreads / 64;
    const float inv_hw = 1.f / (float)HW;
    const float* xb = x + (size_t)b * C * HW;
    for (int c = wave; c < C; c += nwave) {
        const float* row = xb + (size_t)c * HW;
        float acc = 0.f;
        if (vec4) {
            const float4* row4 = reinterpret_cast<const float4*>(row);
            for (int i = lane; i < (HW >> 2); i += 64) {
                const float4 q = row4[i];
                acc += (q.x + q.y) + (q.z + q.w);
            }
        } else {
            for (int i = lane; i < HW; i += 64) acc += row[i];
        }
        acc = wave_sum(acc) * inv_hw;
        if (lane == 0) {
            mean_s[c] = acc;
            means[(size_t)b * C + c] = acc;
        }
    }
    __syncthreads();
    const int nout = 6 * F;
    for (int o = wave; o < nout; o += nwave) {
        const float* wo = w + (size_t)o * C;
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc += wo[c] * mean_s[c];
        acc = wave_sum(acc);
        if (lane == 0) {
            const float p = scale * (acc + (bias ? bias[o] : 0.f));
            par_s[o] = p;
            params[(size_t)b * nout + o] = p;
        }
    }
    if (!T) return;
    __syncthreads();
    if (threadIdx.x < F) {
        const int f = threadIdx.x;
        float M[16];
        pose_transform(par_s + 6 * f, par_s + 6 * f + 3, (invert_mask >> f) & 1, M);
        float* Tb = T + ((size_t)b * F + f) * 16;
#pragma unroll
        for (int k = 0; k < 16; ++k) Tb[k] = M[k];
    }
}

// Backward, launch 1 (one block): g[b, o] = scale * (d_params[b, o] + (d T[b, f] / d params[b, o]) : dT[b, f]), the gradient of the
// unscaled 1x1 output; then dbias[o] = sum_b g[b, o], b ascending.
__global__ void __launch_bounds__(256) pose_head_bwd_params_kernel(const float* __restrict__ params, const float* __restrict__ d_params,
                                                                   const float* __restrict__ dT, float* __restrict__ g,
                                                                   float* __restrict__ dbias, int B, int F, int invert_mask, float scale) {
    const int nout = 6 * F;
    for (int i = threadIdx.x; i < B * F; i += 256) {
        const int f = i % F;
        const float* p = params + (size_t)i * 6;
        float gv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (dT) {
            float G[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) G[k] = dT[(size_t)i * 16 + k];
            pose_transform_bwd(p, p + 3, (invert_mask >> f) & 1, G, gv, gv + 3);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) g[(size_t)i * 6 + k] = scale * (gv[k] + (d_params ? d_params[(size_t)i * 6 + k] : 0.f));
    }
    if (!dbias) return;
    __syncthreads();   // one block: its own global writes are visible to it after the barrier
    if (threadIdx.x < nout) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += g[(size_t)b * nout + threadIdx.x];
        dbias[threadIdx.x] = acc;
    }
}

// Backward, launch 2.  Blocks [0, ndx): image b, a group of kDxChannels channels: dx[b, c, :] = (sum_o g[b, o] w[o, c]) / (H W),
// the mean's gradient spread over the map.  Blocks [ndx, ndx + ndw): 256 channels each: dw[o, c] = sum_b g[b, o] mean[b, c],
// b ascending.
__global__ void __launch_bounds__(256) pose_head_bwd_kernel(const float* __restrict__ g, const float* __restrict__ means,
                                                            const float* __restrict__ w, float* __restrict__ dx, float* __restrict__ dw,
                                                            int B, int C, int HW, int F, int ndx, int groups) {
    __shared__ float val[kDxChannels];
    const int nout = 6 * F;
    if ((int)blockIdx.x < ndx) {
        const int b = blockIdx.x / groups, c0 = (blockIdx.x % groups) * kDxChannels;
        const int nc = min(kDxChannels, C - c0);
        if ((int)threadIdx.x < nc) {
            float acc = 0.f;
            for (int o = 0; o < nout; ++o) acc += g[(size_t)b * nout + o] * w[(size_t)o * C + c0 + threadIdx.x];
            val[threadIdx.x] = acc / (float)HW;
        }
        __syncthreads();
        float* out = dx + ((size_t)b * C + c0) * HW;
        const int n = nc * HW;
        for (int i = threadIdx.x; i < n; i += 256) out[i] = val[i / HW];
        return;
    }
    const int c = ((int)blockIdx.x - ndx) * 256 + threadIdx.x;
    if (c >= C) return;
    float acc[kMaxOut];
#pragma unroll
    for (int o = 0; o < kMaxOut; ++o) acc[o] = 0.f;
    for (int b = 0; b < B; ++b) {
        const float m = means[(size_t)b * C + c];
#pragma unroll
        for (int o = 0; o < kMaxOut; ++o)
            if (o < nout) acc[o] += g[(size_t)b * nout + o] * m;
    }
#pragma unroll
    for (int o = 0; o < kMaxOut; ++o)
        if (o < nout) dw[(size_t)o * C + c] = acc[o];
}

int check_head_shape(const char* fn, int B, int C, int H, int W, int F) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return fail(WMD_ERR_BAD_ARG, "%s: negative size B=%d C=%d H=%d W=%d", fn, B, C, H, W);
    if (F < 1 || F > kMaxFrames) return fail(WMD_ERR_UNSUPPORTED, "%s: F=%d frames, supported 1..%d", fn, F, kMaxFrames);
    if (B == 0 || C == 0 || H == 0 || W == 0) return fail(WMD_ERR_BAD_SHAPE, "%s: empty tensor B=%d C=%d H=%d W=%d", fn, B, C, H, W);
    if ((size_t)(C + kMaxOut) * sizeof(float) > 64 * 1024) return fail(WMD_ERR_UNSUPPORTED, "%s: C=%d channels do not fit the means in LDS", fn, C);
    if ((double)B * C * H * W > 2147483647.0) return fail(WMD_ERR_UNSUPPORTED, "%s: more than 2^31 elements", fn);
    return WMD_OK;
}

}  // namespace
}  // namespace wmd

using namespace wmd;

extern "C" int wmd_pose_transform_fwd(const float* axisangle, const float* translation, float* T, int N, int invert, void* stream) {
    if (!axisangle || !translation || !T) return fail(WMD_ERR_BAD_ARG, "wmd_pose_transform_fwd: null tensor pointer");
    if (N < 0) return fail(WMD_ERR_BAD_ARG, "wmd_pose_transform_fwd: negative N=%d", N);
    if (N == 0) return WMD_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("pose_transform_fwd_kernel", 80.0 * N, 4.0 * 22.0 * N, s);
    hipLaunchKernelGGL(pose_transform_fwd_kernel, dim3((N + 255) / 256), dim3(256), 0, s, axisangle, translation, T, N, invert);
    return check_launch("pose_transform_fwd_kernel");
}

extern "C" int wmd_pose_transform_bwd(const float* axisangle, const float* translation, const float* dT, float* d_axisangle,
                                      float* d_translation, int N, int invert, void* stream) {
    if (!axisangle || !translation || !dT || !d_axisangle || !d_translation)
        return fail(WMD_ERR_BAD_ARG, "wmd_pose_transform_bwd: null tensor pointer");
    if (N < 0) return fail(WMD_ERR_BAD_ARG, "wmd_pose_transform_bwd: negative N=%d", N);
    if (N == 0) return WMD_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("pose_transform_bwd_kernel", 200.0 * N, 4.0 * 28.0 * N, s);
    hipLaunchKernelGGL(pose_transform_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, s, axisangle, translation, dT, d_axisangle,
                       d_translation, N, invert);
    return check_launch("pose_transform_bwd_kernel");
}

extern "C" int wmd_pose_head_fwd(const float* x, const float* w, const float* bias, float* params, float* T, float* means, int B, int C,
                                 int H, int W, int F, int invert_mask, float scale, void* stream) {
    if (!x || !w || !params || !means) return fail(WMD_ERR_BAD_ARG, "wmd_pose_head_fwd: null tensor pointer");
    if (int st = check_head_shape("wmd_pose_head_fwd", B, C, H, W, F)) return st;
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W;
    const int vec4 = (HW % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0);   // every row starts 16-byte aligned
    const double n = (double)B * C;
    ProfScope prof("pose_head_fwd_kernel", n * (HW + 12.0 * F), 4.0 * (n * (HW + 1) + 6.0 * F * C), s);
    hipLaunchKernelGGL(pose_head_fwd_kernel, dim3(B), dim3(kHeadThreads), (size_t)(C + 6 * F) * sizeof(float), s, x, w, bias, params, T,
                       means, C, HW, F, invert_mask, scale, vec4);
    return check_launch("pose_head_fwd_kernel");
}

extern "C" int wmd_pose_head_bwd(const float* params, const float* means, const float* w, const float* d_params, const float* dT,
                                 float* dx, float* dw, float* dbias, float* workspace, int B, int C, int H, int W, int F, int invert_mask,
                                 float scale, void* stream) {
    if (!params || !means || !w || !workspace) return fail(WMD_ERR_BAD_ARG, "wmd_pose_head_bwd: null tensor pointer");
    if (!d_params && !dT) return fail(WMD_ERR_BAD_ARG, "wmd_pose_head_bwd: null d_params and dT (one of them is needed)");
    if (int st = check_head_shape("wmd_pose_head_bwd", B, C, H, W, F)) return st;
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W;
    {
        ProfScope prof("pose_head_bwd_params_kernel", 300.0 * B * F, 4.0 * 34.0 * B * F, s);
        hipLaunchKernelGGL(pose_head_bwd_params_kernel, dim3(1), dim3(256), 0, s, params, d_params, dT, workspace, dbias, B, F,
                           invert_mask, scale);
        if (int st = check_launch("pose_head_bwd_params_kernel")) return st;
    }
    if (!dx && !dw) return WMD_OK;
    const int groups = (C + kDxChannels - 1) / kDxChannels;
    const int ndx = dx ? B * groups : 0, ndw = dw ? (C + 255) / 256 : 0;
    const double n = (double)B * C;
    ProfScope prof("pose_head_bwd_kernel", 24.0 * F * n, 4.0 * (n * (HW + 1) + 12.0 * F * C), s);
    hipLaunchKernelGGL(pose_head_bwd_kernel, dim3(ndx + ndw), dim3(256), 0, s, workspace, means, w, dx, dw, B, C, HW, F, ndx, groups);
    return check_launch("pose_head_bwd_kernel");
}
