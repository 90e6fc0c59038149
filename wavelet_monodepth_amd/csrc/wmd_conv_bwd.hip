// Data gradient of the fused decoder convolution (autograd of ConvBlock/Conv3x3/Conv1x1 + upsample + cat + pad;
// the reference gets it implicitly from torch.autograd, KITTI/trainer.py:211, NYUv2/train.py:327).
//
//   forward:  z = W * P(x1, x2),   P = pad o concat o nearest-upsample   (a linear gather)
//   dgrad:    dP = W^T (*) dz on the padded (H+2)x(W+2) domain  -> conv_fwd_kernel fed with dz, the
//             transposed+flipped weight image and shift1 = 1;   dx = P^T dP  -> conv_dgrad_fold_kernel
//             (reflect/replicate border accumulation, channel split, 2x2 sum for the upsampled source)
// The weight gradient lives in wmd_conv_wgrad.hip / wmd_conv_wgrad32.hip, the depthwise 3x3 in wmd_dwconv.hip (its data
// gradient ends in this file's fold kernel: launch_dgrad_fold).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include "wmd_conv_common.h"

namespace wmd {

// ------------------------------------------------------------------------------------------------
// dgrad stage 2: adjoint of pad + concat + upsample
// ------------------------------------------------------------------------------------------------
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // dword-aligned 16-byte global load

// One (image, channel) plane: out[y, x] = sum of the u x u padded-domain gradients that the forward gather read from
// source pixel (y, x), plus -- on the (rare, divergent) border lines -- the halo rows / columns that reflect or
// replicate padding mirrored onto it.  VEC: a thread owns 4 consecutive padded-domain columns (4/U outputs).
template <int U, bool VEC>
__device__ __forceinline__ void fold_plane(const float* __restrict__ gp, float* __restrict__ op, int H, int W, int pad_mode,
                                           int halo, const float* __restrict__ gate, int gate_act, float gate_slope) {
    constexpr int NX = VEC ? 4 : U;       // padded-domain columns per thread
    constexpr int VX = NX / U;            // outputs per thread
    const int Wp = W + 2 * halo;
    const int h_ = H / U, w_ = W / U, wq = w_ / VX;
    const int lo_src = pad_mode == WMD_PAD_REFLECT ? 1 : 0, hi_src = W - (pad_mode == WMD_PAD_REFLECT ? 2 : 1);
    const int lo_row = lo_src, hi_row = H - (pad_mode == WMD_PAD_REFLECT ? 2 : 1);
    const bool folds = halo && pad_mode != WMD_PAD_ZERO;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < h_ * wq; i += gridDim.x * blockDim.x) {
        const int y = i / wq, xq = i - y * wq;
        const int X0 = xq * NX;
        float o[VX];
#pragma unroll
        for (int e = 0; e < VX; ++e) o[e] = 0.f;
        auto add_row = [&](int r) {
            const float* p = gp + (size_t)r * Wp;
            float v[NX];
            if constexpr (VEC) {
                const f32x4u q = *reinterpret_cast<const f32x4u*>(p + X0 + halo);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < NX; ++e) v[e] = p[X0 + halo + e];
            }
#pragma unroll
            for (int e = 0; e < NX; ++e) {
                float s = v[e];
                if (folds && X0 + e == lo_src) s += p[0];
                if (folds && X0 + e == hi_src) s += p[W + 1];
                o[e / U] += s;
            }
        };
#pragma unroll
        for (int dy = 0; dy < U; ++dy) {
            const int Y = y * U + dy;
            add_row(Y + halo);
            if (folds && Y == lo_row) add_row(0);
            if (folds && Y == hi_row) add_row(H + 1);
        }
        float* dst = op + (size_t)y * w_ + xq * VX;
        if (gate) {   // the source plane is itself an activation output: hand its producer dz = dx * f'(x)
            const float* gq = gate + (size_t)y * w_ + xq * VX;
            float gv[VX];
            if constexpr (VX == 4) {
                const float4 q4 = *reinterpret_cast<const float4*>(gq);
                gv[0] = q4.x, gv[1] = q4.y, gv[2] = q4.z, gv[3] = q4.w;
            } else if constexpr (VX == 2) {
                const float2 q2 = *reinterpret_cast<const float2*>(gq);
                gv[0] = q2.x, gv[1] = q2.y;
            } else {
                gv[0] = gq[0];
            }
#pragma unroll
            for (int e = 0; e < VX; ++e) o[e] *= act_deriv(gv[e], gate_act, gate_slope);
        }
        if constexpr (VX == 4) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        else if constexpr (VX == 2) *reinterpret_cast<float2*>(dst) = make_float2(o[0], o[1]);
        else dst[0] = o[0];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void conv_dgrad_fold_kernel(const float* __restrict__ g, float* __restrict__ dx1,
                                                              float* __restrict__ dx2, int B, int C1, int C2, int H, int W,
                                                              int up1, int pad_mode, int halo, const float* __restrict__ x1_fwd,
                                                              int x1_act, float x1_slope) {
    // blockIdx.y = (image, channel) plane of the padded-domain gradient
    const int Cin = C1 + C2;
    const int b = blockIdx.y / Cin, ch = blockIdx.y % Cin;
    const bool first = ch < C1;
    float* out = first ? dx1 : dx2;
    if (!out) return;
    const int u = first ? up1 : 1;
    const float* gp = g + (size_t)blockIdx.y * (H + 2 * halo) * (W + 2 * halo);
    const size_t ooff = ((size_t)b * (first ? C1 : C2) + (first ? ch : ch - C1)) * (H / u) * (W / u);
    float* op = out + ooff;
    const float* gate = (first && x1_fwd && x1_act != WMD_ACT_NONE) ? x1_fwd + ooff : nullptr;
    if (u == 2) fold_plane<2, VEC>(gp, op, H, W, pad_mode, halo, gate, x1_act, x1_slope);
    else fold_plane<1, VEC>(gp, op, H, W, pad_mode, halo, gate, x1_act, x1_slope);
}

// a thread folds 4 padded-domain columns when rows split into whole quads (dx pointers come 16-byte aligned
// from the caller's allocator; the scalar kernel covers everything else)
void launch_dgrad_fold(const float* g, float* dx1, float* dx2, int B, int C1, int C2, int H, int W, int up1, int pad_mode, int halo,
                       const float* x1_fwd, int x1_act, float x1_slope, hipStream_t s) {
    const bool vec = W % 4 == 0 && ((uintptr_t)dx1 % 16 == 0) && ((uintptr_t)dx2 % 16 == 0);
    const int work = H * W / (vec ? 4 : 1);
    const dim3 grid(std::max(1, std::min((work + 255) / 256, 64)), B * (C1 + C2));
    hipLaunchKernelGGL(vec ? conv_dgrad_fold_kernel<true> : conv_dgrad_fold_kernel<false>, grid, dim3(256), 0, s, g, dx1, dx2, B, C1, C2, H,
                       W, up1, pad_mode, halo, x1_fwd, x1_act, x1_slope);
}

}  // namespace wmd

using namespace wmd;

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static bool dgrad_direct(const wmd_conv_dgrad_args* g) {
    // 1x1 without upsample/concat: the GEMM output IS dx1
    return g->ksize == 1 && g->up1 == 1 && g->C2 == 0 && g->dx1;
}

static void dgrad_conv_args(const wmd_conv_dgrad_args* g, wmd_conv_args* c, float* gbuf, float* ws, size_t ws_floats) {
    const int halo = g->ksize == 3 ? 1 : 0;
    memset(c, 0, sizeof(*c));
    c->B = g->B;
    c->H = g->H + 2 * halo;
    c->W = g->W + 2 * halo;
    c->C1 = g->Cout;  // the reduction runs over the forward's output channels
    c->up1 = 1;
    c->C2 = 0;
    c->Cout = g->C1 + g->C2;  // rows = forward input channels
    c->ksize = g->ksize;
    c->pad_mode = WMD_PAD_ZERO;
    c->act = WMD_ACT_NONE;
    c->x1 = g->dz;
    c->wp = g->wp_dgrad;
    c->wp_wino = g->ksize == 3 ? g->wp_dgrad_wino : nullptr;
    c->y = gbuf;
    c->workspace = ws;
    c->workspace_floats = ws_floats;
    c->tune_cfg = g->tune_cfg;
    c->tune_ksplit = g->tune_ksplit;
    if (dgrad_direct(g) && g->x1_fwd && g->x1_act != WMD_ACT_NONE) {   // the GEMM output IS dx1: gate it in the epilogue
        c->gate = g->x1_fwd;
        c->gate_act = g->x1_act;
        c->gate_slope = g->x1_slope;
    }
}


extern "C" size_t wmd_conv_dgrad_workspace_floats(const wmd_conv_dgrad_args* g) {
    if (!g || g->B <= 0) return 0;
    const int halo = g->ksize == 3 ? 1 : 0;
    const size_t gsz = dgrad_direct(g) ? 0 : (size_t)g->B * (g->C1 + g->C2) * (g->H + 2 * halo) * (g->W + 2 * halo);
    wmd_conv_args c;
    dgrad_conv_args(g, &c, nullptr, nullptr, 0);
    return gsz + wmd_conv_fwd_workspace_floats(&c);
}

extern "C" int wmd_conv_dgrad(const wmd_conv_dgrad_args* g, void* stream) {
    if (!g) return fail(WMD_ERR_BAD_ARG, "wmd_conv_dgrad: null args");
    if (!g->dz || !g->wp_dgrad) return fail(WMD_ERR_BAD_ARG, "wmd_conv_dgrad: null tensor pointer");
    if (!g->dx1 && !g->dx2) return WMD_OK;
    if (g->dx2 && g->C2 <= 0) return fail(WMD_ERR_BAD_ARG, "wmd_conv_dgrad: dx2 given but C2=%d", g->C2);
    int st = conv_check_problem(g->B, g->H, g->W, g->C1, g->up1, g->C2, g->Cout, g->ksize, g->pad_mode, WMD_ACT_NONE, "wmd_conv_dgrad");
    if (st) return st;
    if (g->ksize == 1 && g->up1 == 2) return fail(WMD_ERR_UNSUPPORTED, "wmd_conv_dgrad: 1x1 with upsampled input");
    const int halo = g->ksize == 3 ? 1 : 0;
    const size_t gsz = dgrad_direct(g) ? 0 : (size_t)g->B * (g->C1 + g->C2) * (g->H + 2 * halo) * (g->W + 2 * halo);
    if (g->workspace_floats < gsz || (gsz && !g->workspace))
        return fail(WMD_ERR_WORKSPACE, "wmd_conv_dgrad: workspace %zu < %zu floats", g->workspace_floats, gsz);
    float* gbuf = dgrad_direct(g) ? g->dx1 : g->workspace;
    wmd_conv_args c;
    dgrad_conv_args(g, &c, gbuf, g->workspace ? g->workspace + gsz : nullptr, g->workspace_floats - gsz);
    if (c.workspace_floats == 0) c.workspace = nullptr;
    st = run_conv(&c, halo, g->H, g->W, stream);
    if (st || dgrad_direct(g)) return st;
    const size_t n = (g->dx1 ? (size_t)g->B * g->C1 * (g->H / g->up1) * (g->W / g->up1) : 0) +
                     (g->dx2 ? (size_t)g->B * g->C2 * g->H * g->W : 0);
    ProfScope prof("conv_dgrad_fold_kernel", (double)n, 4.0 * (gsz + n), (hipStream_t)stream);
    launch_dgrad_fold(gbuf, g->dx1, g->dx2, g->B, g->C1, g->C2, g->H, g->W, g->up1, g->pad_mode, halo, g->x1_fwd, g->x1_act, g->x1_slope,
                      (hipStream_t)stream);
    return check_launch("conv_dgrad_fold_kernel");
}
