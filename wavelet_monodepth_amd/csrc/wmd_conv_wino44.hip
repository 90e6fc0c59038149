// Winograd F(4x4,3x3) trunk convolution in the classical three-pass form, for the COARSE up+skip layers (include/wmd.h,
// wmd_conv_wino44_fwd):
//
//   wino44_input_kernel    V[p][c][tile] = (B^T d B)[p]      6x6 patch of channel c around a 4x4 output tile, 36 positions p
//   wino44_gemm_kernel     M[p][co][tile] = sum_c U[p][c][co] V[p][c][tile]     36 GEMMs on v_mfma_f32_32x32x2_f32
//   wino44_output_kernel   y = act(A^T M A + bias)           16 outputs per (tile, out channel), 16-byte stores
//
// Same operator as wmd_conv_fwd (nearest x2 upsample of x1, channel concat with x2, reflect / replicate / zero border, bias,
// activation), 36 matrix-pipe positions per 16 outputs instead of the 64 of the fused F(2x2,3x3) kernels.  The fused kernels
// carry their input transform on the lanes that issue the MFMAs; here the transforms are passes of their own over V and M in
// the caller's workspace, which only pays where those images are small against the arithmetic: few pixels, many channels.
//
// Points 0, +-1, +-2, inf:
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// Upsampled operand (up1 = 2): a 6-sample line of a 2x-replicated signal is (a, b, b, c, c, e), so B^T d = (4a - 5b + c,
// -8b + 2c, 0, -3(b - c), b - c, 4b - 5c + e): 1-D position 2 is identically 0, so 25 of the 36 positions carry the upsampled
// channels, computed from the operand at its own resolution (a 4x4 patch per tile).  Positions 3 and 4 hold the same datum up to
// the factor -3 but cannot share one GEMM: columns 3 and 4 of A are (1, 2, 4, 8) and (1, -2, 4, -8), so the even output rows
// need U4 - 3 U3 and the odd ones -(U4 + 3 U3) -- two weight rows either way.  a .. e are the samples 2t-1 .. 2t+2 of the low-
// resolution line, clamped into it (reflect and replicate borders of the upsampled image both land on the edge sample) or 0
// outside it under zero padding.
//
// Images (floats; C1p, C2p = channel counts rounded up to kKC, Coutp = Cout rounded up to 32, NTp = tiles rounded up to 32):
//   U [36][(C1p + C2p) / 4][Coutp][4]   weight image, zero in every padded row / column (wmd_conv_pack_weights_wino44)
//   V [36][(C1p + C2p) / 4][NTp][4]     channels of the upsampled operand exist at its 25 positions only (the others are never touched)
//   M [36][Coutp][NTp]
// U and V keep four consecutive channels innermost: a lane's operands of four successive MFMA k-steps are one 16-byte LDS read
// (lane half h of k-step q of an 8-channel group multiplies channel 4 h + q), 0.5 reads per MFMA instead of 2 -- on this part
// the vector ALU, the LDS issue and the fp32 MFMA share their cycles.
// The channel order of the reduction is fixed (x1's channels, then x2's; one block runs the whole loop): a launch repeats
// bit for bit.
#include <algorithm>
#include "wmd_conv_common.h"

namespace wmd {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKC = 32;    // channels per staged chunk of the GEMM, and the padding unit of both channel counts
constexpr int kBM = 64;    // out channels per GEMM block
constexpr int kBNMax = 128;   // tiles per GEMM block: 128 (reduction over x2 only / pure layers) or 64 (x1 and x2)
constexpr int kGemmLdsFloats = 2 * kKC * (kBM + kBNMax);

struct W44Args {
    const float* x1;
    const float* x2;
    const float* U;
    const float* bias;
    float* V;
    float* M;
    float* y;
    int B, H, W, H1, W1, C1, C2, C1p, Ktot, Cout, Coutp;
    int up, pad_mode, act;
    float slope;
    int th, tw, NT, NTp;
    // GEMM work order: with an upsampled operand 25 "long" positions reduce over x1 and x2 (blocks of 64 tiles) and 11 over x2 only
    // (blocks of 128 tiles: every block is the same work); otherwise all 36 reduce over everything in blocks of 128 tiles.
    // xpos[x]: the positions whose blocks run on XCD x, long ones first; bit 7 marks a long position
    int split, nbm, nbn_long, nbn_short;
    unsigned char xcnt[8];
    unsigned char xpos[8][8];
};

__host__ __device__ constexpr bool up_pos1(int i) { return i != 2; }   // 1-D positions an upsampled line reaches

// one line of B^T d
__device__ __forceinline__ void bt6(const float d[6], float t[6]) {
    const float e42 = d[4] - 4.f * d[2], e31 = d[3] - 4.f * d[1], f42 = d[4] - d[2], f31 = 2.f * (d[3] - d[1]);
    t[0] = (4.f * d[0] - 5.f * d[2]) + d[4];
    t[1] = e42 + e31;
    t[2] = e42 - e31;
    t[3] = f42 + f31;
    t[4] = f42 - f31;
    t[5] = (4.f * d[1] - 5.f * d[3]) + d[5];
}
// the five data terms of a replicated line (a, b, b, c, c, e): positions 0, 1, 3, 4, 5
__device__ __forceinline__ void bt5(const float s[4], float t[5]) {
    const float bc = s[1] - s[2];
    t[0] = (4.f * s[0] - 5.f * s[1]) + s[2];
    t[1] = 2.f * s[2] - 8.f * s[1];
    t[2] = -3.f * bc;
    t[3] = bc;
    t[4] = (4.f * s[1] - 5.f * s[2]) + s[3];
}

// thread = (channel c, tile); the four channels of a V group are neighbouring lanes: every store instruction writes whole lines
__global__ __launch_bounds__(256) void wino44_input_kernel(const W44Args a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int tile = (idx >> 2) % a.NTp, c = ((idx >> 2) / a.NTp) * 4 + (idx & 3);   // a wave: 16 tiles x 4 channels = 256 bytes of V per store
    if (c >= a.Ktot) return;
    const bool op1 = c < a.C1p;
    const bool structured = op1 && a.up == 2;
    const int ch = op1 ? c : c - a.C1p;
    const bool live = tile < a.NT && ch < (op1 ? a.C1 : a.C2);
    const size_t pstride = (size_t)a.Ktot * a.NTp;
    float* vout = a.V + ((size_t)(c >> 2) * a.NTp + tile) * 4 + (c & 3);
    const int tx = tile % a.tw, ty = (tile / a.tw) % a.th, b = tile / (a.tw * a.th);
    if (structured) {
        float s[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[i][j] = 0.f;
        if (live) {
            const float* src = a.x1 + ((size_t)b * a.C1 + ch) * a.H1 * a.W1;
            int ro[4], co[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r0 = 2 * ty - 1 + i, r = min(max(r0, 0), a.H1 - 1);
                ro[i] = (a.pad_mode == WMD_PAD_ZERO && r != r0) ? -1 : r * a.W1;
                const int c0 = 2 * tx - 1 + i, cc = min(max(c0, 0), a.W1 - 1);
                co[i] = (a.pad_mode == WMD_PAD_ZERO && cc != c0) ? -1 : cc;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((ro[i] | co[j]) >= 0) s[i][j] = src[ro[i] + co[j]];
        }
        float t[5][4];   // [position row][source column]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float col[4] = {s[0][j], s[1][j], s[2][j], s[3][j]};
            float r[5];
            bt5(col, r);
#pragma unroll
            for (int i = 0; i < 5; ++i) t[i][j] = r[i];
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            float r[5];
            bt5(t[i], r);
            const int pi = i < 2 ? i : i + 1;
#pragma unroll
            for (int j = 0; j < 5; ++j) vout[(size_t)(pi * 6 + (j < 2 ? j : j + 1)) * pstride] = r[j];
        }
        return;
    }
    float d[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) d[i][j] = 0.f;
    if (live) {
        const float* src = op1 ? a.x1 + ((size_t)b * a.C1 + ch) * a.H * a.W : a.x2 + ((size_t)b * a.C2 + ch) * a.H * a.W;
        int ro[6], co[6];
        // padded coordinate g in [-1, n + 3]: beyond n only discarded outputs of a ragged tile are reached (read 0)
        // (not pad_fold, wmd_internal.h: that one clears a flag and returns an in-range pixel; this one answers -1 for "reads 0", also beyond n)
        auto fold = [&](int g, int n) {
            const int refl = g < 0 ? -g : (g >= n ? 2 * n - 2 - g : g);
            const int clam = min(max(g, 0), n - 1);
            if (g > n || (a.pad_mode == WMD_PAD_ZERO && g != clam)) return -1;
            return min(max(a.pad_mode == WMD_PAD_REFLECT ? refl : clam, 0), n - 1);
        };
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int r = fold(4 * ty - 1 + i, a.H);
            ro[i] = r < 0 ? -1 : r * a.W;
            co[i] = fold(4 * tx - 1 + i, a.W);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if ((ro[i] | co[j]) >= 0) d[i][j] = src[ro[i] + co[j]];
    }
    float t[6][6];   // [position row][source column]
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float col[6] = {d[0][j], d[1][j], d[2][j], d[3][j], d[4][j], d[5][j]};
        float r[6];
        bt6(col, r);
#pragma unroll
        for (int i = 0; i < 6; ++i) t[i][j] = r[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float r[6];
        bt6(t[i], r);
#pragma unroll
        for (int j = 0; j < 6; ++j) vout[(size_t)(i * 6 + j) * pstride] = r[j];
    }
}

// One GEMM block: kBM out channels x BN tiles of position p, channels [kbeg, Ktot).  Four waves, wave (wm, wn) owns out channels
// 32 wm .. +32 (MFMA rows: A = U) and tiles (BN/2) wn .. +BN/2 (MFMA columns: B = V).  Both operands are [channel / 4][row][4] in
// memory, so a chunk of kKC channels is kKC / 4 runs of 16 kBM / 16 BN bytes: 16-byte LDS-DMA pieces, the LDS image is the same
// [group][row][4], and the operands of four k-steps are one ds_read_b128 (32 lanes read 512 contiguous bytes: no bank conflicts).
// A run that crosses the end of its group (Coutp % 64, NTp % BN) continues into the next group or -- past the buffer -- reads 0
// through the buffer resource: those rows / columns of the product are not stored.  An upsampled layer without a skip tensor has no
// channels left at the 11 positions its operand does not reach: no chunk, M = 0.
template <int BN>
__device__ __forceinline__ void w44_gemm_tile(const W44Args& a, float* lds, int p, int kbeg, int m0, int n0) {
    constexpr int NJ = BN / 64;                   // 32x32 accumulator tiles per wave
    constexpr int NG = kKC / 4;                   // channel groups per chunk
    constexpr int A_FLOATS = kKC * kBM, B_FLOATS = kKC * BN, BUF = A_FLOATS + B_FLOATS;
    constexpr int NPA = A_FLOATS / 4 / 256, NPB = B_FLOATS / 4 / 256;   // 16-byte pieces per thread and chunk
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv & 1, wn = wv >> 1;

    const float* Up = a.U + (size_t)p * a.Ktot * a.Coutp;
    const float* Vp = a.V + (size_t)p * a.Ktot * a.NTp;
    const size_t u_left = (size_t)(36 - p) * a.Ktot * a.Coutp * 4, v_left = (size_t)(36 - p) * a.Ktot * a.NTp * 4;   // < 2^31: host check
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Up), 0, (int)u_left, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Vp), 0, (int)v_left, 0x00020000);
    unsigned offA[NPA], offB[NPB];   // byte offset of piece e = tid + 256 i inside a chunk: group e / rows, 16-byte piece e % rows of the block's run
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
        const int e = tid + i * 256, grp = e / kBM, row = e % kBM;
        offA[i] = (unsigned)(((grp * a.Coutp + m0 + row) * 4) * 4);
    }
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
        const int e = tid + i * 256, grp = e / BN, row = e % BN;
        offB[i] = (unsigned)(((grp * a.NTp + n0 + row) * 4) * 4);
    }
    // (the chunk offset travels in the per-lane offset: the resource's range check does not cover a scalar offset)
    auto stage = [&](int c0, float* buf) {
        const unsigned sa = (unsigned)c0 * (unsigned)a.Coutp * 4u, sb = (unsigned)c0 * (unsigned)a.NTp * 4u;
#pragma unroll
        for (int i = 0; i < NPA; ++i) lds_dma16(ru, (lds_ptr_t)(buf + (wv * 64 + i * 256) * 4), offA[i] + sa, 0);
#pragma unroll
        for (int i = 0; i < NPB; ++i) lds_dma16(rv, (lds_ptr_t)(buf + A_FLOATS + (wv * 64 + i * 256) * 4), offB[i] + sb, 0);
    };

    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int nchunks = (a.Ktot - kbeg) / kKC;
    if (nchunks > 0) stage(kbeg, lds);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // lane half h = lane >> 5 reads group 2 gp + h of the chunk: channels 8 gp + 4 h + q for k-step q
    const int aoff = ((lane >> 5) * kBM + wm * 32 + (lane & 31)) * 4;
    const int boff = A_FLOATS + ((lane >> 5) * BN + wn * (BN / 2) + (lane & 31)) * 4;
    for (int ch = 0; ch < nchunks; ++ch) {
        const float* buf = lds + (ch & 1) * BUF;
        if (ch + 1 < nchunks) stage(kbeg + (ch + 1) * kKC, lds + ((ch + 1) & 1) * BUF);
#pragma unroll
        for (int gp = 0; gp < NG / 2; ++gp) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(buf + aoff + gp * 2 * kBM * 4);
            f32x4 bv[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bv[j] = *reinterpret_cast<const f32x4*>(buf + boff + (gp * 2 * BN + j * 32) * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[j][q], acc[j], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next chunk has landed ...
        __syncthreads();                                    // ... for everybody, and this buffer is free
    }

    // accumulator register r of lane l: out channel 8 (r / 4) + 4 (l >> 5) + r % 4, tile l & 31 -- a register is a 128-byte line of M
    float* Mp = a.M + (size_t)p * a.Coutp * a.NTp;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int tile = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = m0 + wm * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
            if (co < a.Coutp && tile < a.NTp) Mp[(size_t)co * a.NTp + tile] = acc[j][r];
        }
    }
}

// Work order: workgroup id % 8 is the XCD a block runs on.  Every position's blocks -- which share its U and V slices -- run on one
// XCD and meet in one L2; the host deals the positions to the XCDs (most work first, to the least loaded), long ones first.
__global__ __launch_bounds__(256, 3) void wino44_gemm_kernel(const W44Args a) {
    __shared__ __attribute__((aligned(16))) float lds[kGemmLdsFloats];
    const int xcd = blockIdx.x & 7;
    int j = blockIdx.x >> 3;
    const int nb_long = a.nbm * a.nbn_long, nb_short = a.nbm * a.nbn_short;
    for (int sl = 0; sl < a.xcnt[xcd]; ++sl) {
        const int e = a.xpos[xcd][sl], p = e & 63;
        const bool lng = (e & 128) != 0;
        const int nb = lng ? nb_long : nb_short;
        if (j < nb) {
            if (lng) w44_gemm_tile<64>(a, lds, p, 0, (j % a.nbm) * kBM, (j / a.nbm) * 64);
            else w44_gemm_tile<128>(a, lds, p, a.split ? a.C1p : 0, (j % a.nbm) * kBM, (j / a.nbm) * 128);
            return;
        }
        j -= nb;
    }
}

// thread = (out channel, tile), tile fastest: 36 coalesced reads of M, four rows of 16 bytes of y
template <int ACT>
__device__ __forceinline__ void w44_store(const W44Args& a, const float m[6][6], int co, int b, int ty, int tx) {
    // rows: P = A^T M (4 x 6), then Y = P A
    float y[4][4];
    float pr[4][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float s12 = m[1][j] + m[2][j], d12 = m[1][j] - m[2][j], s34 = m[3][j] + m[4][j], d34 = m[3][j] - m[4][j];
        pr[0][j] = (m[0][j] + s12) + s34;
        pr[1][j] = d12 + 2.f * d34;
        pr[2][j] = s12 + 4.f * s34;
        pr[3][j] = (d12 + 8.f * d34) + m[5][j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float s12 = pr[i][1] + pr[i][2], d12 = pr[i][1] - pr[i][2], s34 = pr[i][3] + pr[i][4], d34 = pr[i][3] - pr[i][4];
        y[i][0] = (pr[i][0] + s12) + s34;
        y[i][1] = d12 + 2.f * d34;
        y[i][2] = s12 + 4.f * s34;
        y[i][3] = (d12 + 8.f * d34) + pr[i][5];
    }
    const float bv = a.bias ? a.bias[co] : 0.f;
    const int x0 = 4 * tx;
    const bool vec = (a.W & 3) == 0;   // then every tile is four whole columns and every row start is 16-byte aligned
    float* dst = a.y + (((size_t)b * a.Cout + co) * a.H + 4 * ty) * a.W + x0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (4 * ty + i >= a.H) break;
        const f32x2 o0 = w32_act2<ACT>(f32x2{y[i][0], y[i][1]} + f32x2{bv, bv}, a.slope);
        const f32x2 o1 = w32_act2<ACT>(f32x2{y[i][2], y[i][3]} + f32x2{bv, bv}, a.slope);
        if (vec) *reinterpret_cast<float4*>(dst + (size_t)i * a.W) = make_float4(o0[0], o0[1], o1[0], o1[1]);
        else {
            const float o[4] = {o0[0], o0[1], o1[0], o1[1]};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x0 + e < a.W) dst[(size_t)i * a.W + e] = o[e];
        }
    }
}

__global__ __launch_bounds__(256) void wino44_output_kernel(const W44Args a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int tile = idx % a.NTp, co = idx / a.NTp;
    if (co >= a.Cout || tile >= a.NT) return;
    const int tx = tile % a.tw, ty = (tile / a.tw) % a.th, b = tile / (a.tw * a.th);
    const size_t pstride = (size_t)a.Coutp * a.NTp;
    const float* src = a.M + (size_t)co * a.NTp + tile;
    float m[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) m[i][j] = src[(size_t)(i * 6 + j) * pstride];
    if (a.act == WMD_ACT_ELU) w44_store<WMD_ACT_ELU>(a, m, co, b, ty, tx);
    else if (a.act == WMD_ACT_LEAKY) w44_store<WMD_ACT_LEAKY>(a, m, co, b, ty, tx);
    else if (a.act == WMD_ACT_SIGMOID) w44_store<WMD_ACT_SIGMOID>(a, m, co, b, ty, tx);
    else w44_store<WMD_ACT_NONE>(a, m, co, b, ty, tx);
}

// U = G g G^T in double, rounded once; rows of an upsampled operand are 0 at the 11 positions it does not reach
__global__ __launch_bounds__(256) void wino44_pack_kernel(const float* __restrict__ w, float* __restrict__ U, int Cout, int C1, int C2,
                                                          int C1p, int Ktot, int Coutp, int up) {
    const double G[6][3] = {{0.25, 0.0, 0.0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                            {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0.0, 0.0, 1.0}};
    const size_t total = (size_t)36 * Ktot * Coutp;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int co = (int)((i >> 2) % Coutp);   // [p][c / 4][co][c % 4]
        const int c = (int)(((i >> 2) / Coutp) % (Ktot / 4)) * 4 + (int)(i & 3), p = (int)(i / ((size_t)Coutp * Ktot));
        const bool op1 = c < C1p;
        const int ch = op1 ? c : c - C1p;
        const bool structured = op1 && up == 2;
        const int pi = p / 6, pj = p % 6;
        float out = 0.f;
        if (co < Cout && ch < (op1 ? C1 : C2) && (!structured || (up_pos1(pi) && up_pos1(pj)))) {
            const float* g = w + ((size_t)co * (C1 + C2) + (op1 ? ch : C1 + ch)) * 9;
            double s = 0.0;
            for (int ii = 0; ii < 3; ++ii)
                for (int jj = 0; jj < 3; ++jj) s += G[pi][ii] * (double)g[ii * 3 + jj] * G[pj][jj];
            out = (float)s;
        }
        U[i] = out;
    }
}

struct W44Dims {
    int C1p, C2p, Ktot, Coutp, th, tw, NT, NTp;
    size_t u_floats, v_floats, m_floats;
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

W44Dims w44_dims(int B, int H, int W, int C1, int C2, int Cout) {
    W44Dims d;
    d.C1p = round_up(C1, kKC);
    d.C2p = round_up(C2, kKC);
    d.Ktot = d.C1p + d.C2p;
    d.Coutp = round_up(Cout, 32);
    d.th = (H + 3) / 4;
    d.tw = (W + 3) / 4;
    const long long nt = (long long)B * d.th * d.tw;
    d.NT = (int)std::min<long long>(nt, 1 << 28);
    d.NTp = round_up(d.NT, 32);
    d.u_floats = (size_t)36 * d.Ktot * d.Coutp;
    d.v_floats = (size_t)36 * d.Ktot * d.NTp;
    d.m_floats = (size_t)36 * d.Coutp * d.NTp;
    return d;
}

constexpr size_t kMaxImageBytes = (size_t)1 << 31;   // 32-bit byte offsets inside every image

// the problem alone -- the operator's contract, then which optional features are asked for (a mask, a gate, a tile list: by
// being non-null) and the family's limits; no tensor pointer is required: what wmd_conv_wino44_supported / _workspace_floats answer from
int w44_validate(const wmd_conv_args* g, const char* who) {
    if (!g) return fail(WMD_ERR_BAD_ARG, "%s: null args", who);
    const int st = conv_check_problem(g->B, g->H, g->W, g->C1, g->up1, g->C2, g->Cout, g->ksize, g->pad_mode, g->act, who);
    if (st) return st;
    if (g->ksize != 3) return fail(WMD_ERR_UNSUPPORTED, "%s: ksize=%d (3x3 only)", who, g->ksize);
    if (g->gate) return fail(WMD_ERR_UNSUPPORTED, "%s: gate is not implemented by the F(4x4,3x3) kernels", who);
    if (g->in_mask || g->out_mask || g->out_tiles || g->out_tile_count)
        return fail(WMD_ERR_UNSUPPORTED, "%s: in_mask / out_mask / out_tiles are not implemented by the F(4x4,3x3) kernels", who);
    if (g->tune_cfg != 0 || g->tune_ksplit != 0)
        return fail(WMD_ERR_UNSUPPORTED, "%s: tune_cfg=%d tune_ksplit=%d (one configuration, no split)", who, g->tune_cfg, g->tune_ksplit);
    if ((long long)g->B * ((g->H + 3) / 4) * ((g->W + 3) / 4) > (1 << 24) || g->C1 > (1 << 16) || g->C2 > (1 << 16) || g->Cout > (1 << 16))
        return fail(WMD_ERR_UNSUPPORTED, "%s: more than 2^24 tiles or 2^16 channels", who);
    const W44Dims d = w44_dims(g->B, g->H, g->W, g->C1, g->C2, g->Cout);
    const size_t hw = (size_t)g->H * g->W;
    if (d.u_floats * 4 >= kMaxImageBytes || d.v_floats * 4 >= kMaxImageBytes || d.m_floats * 4 >= kMaxImageBytes ||
        (size_t)d.Ktot * d.NTp >= kMaxImageBytes / 4 || (size_t)g->B * g->Cout * hw * 4 >= kMaxImageBytes ||
        (size_t)g->B * std::max(g->C1, g->C2) * hw * 4 >= kMaxImageBytes)
        return fail(WMD_ERR_UNSUPPORTED, "%s: a tensor, the weight image or a workspace image exceeds 2 GiB", who);
    return WMD_OK;
}

}  // namespace
}  // namespace wmd

using namespace wmd;

extern "C" size_t wmd_conv_packed_weight_floats_wino44(int Cout, int C1, int C2) {
    if (Cout < 1 || C1 < 1 || C2 < 0 || Cout > (1 << 16) || C1 > (1 << 16) || C2 > (1 << 16)) return 0;
    return w44_dims(1, 4, 4, C1, C2, Cout).u_floats;
}

extern "C" int wmd_conv_pack_weights_wino44(const float* w, float* wp, int Cout, int C1, int C2, int up1, void* stream) {
    if (!w || !wp) return fail(WMD_ERR_BAD_ARG, "wmd_conv_pack_weights_wino44: null pointer");
    if (up1 != 1 && up1 != 2) return fail(WMD_ERR_BAD_ARG, "wmd_conv_pack_weights_wino44: up1=%d", up1);
    const size_t total = wmd_conv_packed_weight_floats_wino44(Cout, C1, C2);
    if (!total) return fail(WMD_ERR_BAD_SHAPE, "wmd_conv_pack_weights_wino44: Cout=%d C1=%d C2=%d", Cout, C1, C2);
    const W44Dims d = w44_dims(1, 4, 4, C1, C2, Cout);
    ProfScope prof("wino44_pack_kernel", 0.0, 4.0 * total + 36.0 * Cout * (C1 + C2), (hipStream_t)stream);
    hipLaunchKernelGGL(wino44_pack_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       w, wp, Cout, C1, C2, d.C1p, d.Ktot, d.Coutp, up1);
    return check_launch("wino44_pack_kernel");
}

extern "C" int wmd_conv_wino44_supported(const wmd_conv_args* g) { return w44_validate(g, "wmd_conv_wino44_fwd") == WMD_OK; }

extern "C" size_t wmd_conv_wino44_workspace_floats(const wmd_conv_args* g) {
    if (w44_validate(g, "wmd_conv_wino44_fwd") != WMD_OK) return 0;
    const W44Dims d = w44_dims(g->B, g->H, g->W, g->C1, g->C2, g->Cout);
    return d.v_floats + d.m_floats;
}

extern "C" int wmd_conv_wino44_fwd(const wmd_conv_args* g, void* stream) {
    const char* who = "wmd_conv_wino44_fwd";
    int rc = w44_validate(g, who);
    if (rc == WMD_OK) rc = conv_check_tensors(g, who);
    if (rc != WMD_OK) return rc;
    const W44Dims d = w44_dims(g->B, g->H, g->W, g->C1, g->C2, g->Cout);
    if (!g->workspace || g->workspace_floats < d.v_floats + d.m_floats)
        return fail(WMD_ERR_WORKSPACE, "%s: needs a workspace of %zu floats (got %zu)", who, d.v_floats + d.m_floats,
                    g->workspace ? g->workspace_floats : (size_t)0);
    hipStream_t s = (hipStream_t)stream;
    W44Args a;
    a.x1 = g->x1, a.x2 = g->x2, a.U = g->wp, a.bias = g->bias;
    a.V = g->workspace, a.M = g->workspace + d.v_floats, a.y = g->y;
    a.B = g->B, a.H = g->H, a.W = g->W, a.H1 = g->H / g->up1, a.W1 = g->W / g->up1;
    a.C1 = g->C1, a.C2 = g->C2, a.C1p = d.C1p, a.Ktot = d.Ktot, a.Cout = g->Cout, a.Coutp = d.Coutp;
    a.up = g->up1, a.pad_mode = g->pad_mode, a.act = g->act, a.slope = g->slope;
    a.th = d.th, a.tw = d.tw, a.NT = d.NT, a.NTp = d.NTp;
    const bool split = g->up1 == 2;   // two classes of positions: 25 reduce over x1 and x2, 11 over x2 only
    a.split = split;
    a.nbm = (d.Coutp + kBM - 1) / kBM;
    a.nbn_long = (d.NTp + 63) / 64;
    a.nbn_short = (d.NTp + 127) / 128;
    long long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // blocks x chunks dealt to each XCD
    for (int x = 0; x < 8; ++x) a.xcnt[x] = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int p = 0; p < 36; ++p) {
            const bool lng = split && up_pos1(p / 6) && up_pos1(p % 6);
            if (lng != (pass == 0)) continue;
            int x = -1;
            for (int k = 0; k < 8; ++k)
                if (a.xcnt[k] < 8 && (x < 0 || load[k] < load[x])) x = k;   // (8 slots x 8 XCDs >= 36 positions)
            a.xpos[x][a.xcnt[x]++] = (unsigned char)(p | (lng ? 128 : 0));
            load[x] += 1 + (lng ? (long long)a.nbm * a.nbn_long * d.Ktot : (long long)a.nbm * a.nbn_short * (split ? d.C2p : d.Ktot));
        }
    int per_xcd = 0;
    for (int x = 0; x < 8; ++x) {
        int nb = 0;
        for (int k = 0; k < a.xcnt[x]; ++k) nb += a.nbm * ((a.xpos[x][k] & 128) ? a.nbn_long : a.nbn_short);
        per_xcd = std::max(per_xcd, nb);
    }
    const double pix = (double)g->B * g->H * g->W, tiles = d.NT;
    const double krows = split ? 25.0 * d.Ktot + 11.0 * d.C2p : 36.0 * d.Ktot;   // channel rows of V (and U) over all positions
    {
        const double in_bytes = 4.0 * g->B * ((double)g->C1 * a.H1 * a.W1 + (double)g->C2 * g->H * g->W);
        ProfScope prof("wino44_input_kernel", 0.0, in_bytes + 4.0 * krows * d.NTp, s);
        hipLaunchKernelGGL(wino44_input_kernel, dim3((unsigned)(((size_t)d.Ktot * d.NTp + 255) / 256)), dim3(256), 0, s, a);
        const int lrc = check_launch("wino44_input_kernel");
        if (lrc) return lrc;
    }
    {
        // executed: whole blocks of kBM out channels x 64 / 128 tiles
        const double mf = 2.0 * kBM * a.nbm * (split ? 25.0 * d.Ktot * 64 * a.nbn_long + 11.0 * d.C2p * 128 * a.nbn_short
                                                     : 36.0 * d.Ktot * 128 * a.nbn_short);
        ProfScope prof("wino44_gemm_kernel", 2.0 * pix * g->Cout * (g->C1 + g->C2) * 9, 4.0 * (krows * (d.NTp + d.Coutp) + 36.0 * d.Coutp * d.NTp), s);
        prof.mfma(mf);
        hipLaunchKernelGGL(wino44_gemm_kernel, dim3((unsigned)(8 * per_xcd)), dim3(256), 0, s, a);
        const int lrc = check_launch("wino44_gemm_kernel");
        if (lrc) return lrc;
    }
    {
        ProfScope prof("wino44_output_kernel", 0.0, 4.0 * (36.0 * g->Cout * tiles + pix * g->Cout), s);
        hipLaunchKernelGGL(wino44_output_kernel, dim3((unsigned)(((size_t)g->Cout * d.NTp + 255) / 256)), dim3(256), 0, s, a);
        return check_launch("wino44_output_kernel");
    }
}
