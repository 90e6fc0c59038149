// Weight gradient of the fused decoder convolution (autograd of ConvBlock/Conv3x3/Conv1x1 + upsample + cat + pad).
//
//   forward:  z = W * P(x1, x2),   P = pad o concat o nearest-upsample   (a linear gather)
//   wgrad:    dW[co,ci,t] = sum_{b,y,x} dz[b,co,y,x] * P[b,ci,y+ky,x+kx]  -> conv_wgrad_kernel: an MFMA GEMM
//             with M = co, N = (ci,tap), K = pixels; every block owns a (co-tile, ci-tile) pair and a slice
//             of the pixel tiles, accumulates in registers and writes ONE partial; a second kernel sums the
//             partials (deterministic two-stage reduction, no atomics).
//   dbias:    row sums of the dz tiles the wgrad blocks already hold in LDS, reduced with the weight partials.
// The 3x3 layers mostly run the same GEMM in the Winograd F(2x2,3x3) domain: conv_wgrad_wino_kernel here (16x16x4 MFMAs),
// conv_wgrad_wino32_kernel in wmd_conv_wgrad32.hip (32x32x2).  One table type, one plan and one launch path serve them all.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include "wmd_conv_common.h"

namespace wmd {

__device__ __forceinline__ void wg_dma4(__amdgpu_buffer_rsrc_t r, lds_ptr_t dst, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst, 4, voff, soff, 0, 0);
}

// Shared by conv_wgrad_kernel and conv_wgrad_wino_kernel (their staging and partial-slice addressing stay written out in
// each: as helpers they change the kernels' generated code).
// pixel tiles [t_begin, t_end) of partial slice `split`
__device__ __forceinline__ void wg_split_range(const WgradKArgs& a, int split, int& t_begin, int& t_end) {
    const int per = (a.ntiles + a.nsplit - 1) / a.nsplit;
    t_begin = split * per;
    t_end = min(t_begin + per, a.ntiles);
}
// bias partial: the sum of the NPIX staged dz values of one out channel
template <int NPIX>
__device__ __forceinline__ float wg_row_sum(const float* row) {
    float s = 0.f;
    for (int p = 0; p < NPIX; ++p) s += row[p];
    return s;
}

// Block = WM x WN waves. Wave (wm, wn) owns MR out-channel tiles (16 each) x NC 16-input-channel groups x TAPS.
// Pixel tile = TH x TW (TW % 4 == 0): the MFMA K index walks 4 consecutive pixels of a row.
// Both operand tiles are gathered by LDS-DMA (position-linear rows), double buffered across pixel tiles.
template <int TH, int TW, int MR, int NC, int WM, int WN, int TAPS>
struct WgradTile {
    static constexpr int NT = WM * WN * 64;
    static constexpr int HALO = TAPS == 9 ? 1 : 0;
    static constexpr int PH = TH + 2 * HALO, PW = TW + 2 * HALO;
    static constexpr int NPIX = TH * TW;
    static constexpr int NPATCH = PH * PW;
    static constexpr int COT = WM * MR * 16;        // out channels per block
    static constexpr int CIT = WN * NC * 16;        // in channels per block
    // row strides: >= the DMA span (whole 64-lane pieces) and == 2 (mod 32) so that lanes (i = l&15, k = l>>4) of a
    // 32-lane ds_read_b32 group hit banks 2i + k, all distinct
    static constexpr int SPAN_A = ((NPIX + 63) / 64) * 64;
    static constexpr int SPAN_B = ((NPATCH + 63) / 64) * 64;
    static constexpr int SA = ((SPAN_A - 2 + 31) / 32) * 32 + 2;
    static constexpr int SB = ((SPAN_B - 2 + 31) / 32) * 32 + 2;
    static constexpr int BUF = COT * SA + CIT * SB;
    static constexpr int LDS_FLOATS = 2 * BUF;
    static constexpr int PA = SPAN_A / 64, PB = SPAN_B / 64;   // 64-lane DMA pieces per row
    static_assert(TW % 4 == 0, "pixel quads must not straddle rows");
};

template <int TH, int TW, int MR, int NC, int WM, int WN, int TAPS>
__global__ __launch_bounds__(WM* WN * 64) void conv_wgrad_kernel(const WgradKArgs a) {
    using T = WgradTile<TH, TW, MR, NC, WM, WN, TAPS>;
    constexpr int HALO = T::HALO, PW = T::PW, SA = T::SA, SB = T::SB, NPIX = T::NPIX;
    constexpr int NWAVES = WM * WN;
    constexpr unsigned kOOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int co0 = blockIdx.y * T::COT, ci0 = blockIdx.x * T::CIT;
    const int split = blockIdx.z;
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W, plane1 = (size_t)a.H1 * a.W1;
    const unsigned pbz = (unsigned)(plane * 4), pb1 = (unsigned)(plane1 * 4);

    f32x4 acc[MR][NC][TAPS];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < NC; ++n)
#pragma unroll
            for (int t = 0; t < TAPS; ++t) acc[m][n][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;  // bias partial: thread c < COT sums row c of the dz tiles (ci-tile 0 blocks only)

    int t_begin, t_end;
    wg_split_range(a, split, t_begin, t_end);

    // DMA of one pixel tile into buffer `buf`: rows of dz (out channels) and of the gathered input patch.
    // Rows are handed round-robin to the waves; a row is PA (PB) pieces of 64 consecutive positions.
    auto stage = [&](int tile, int buf) {
        int t = tile;
        const int tx = t % a.tiles_x;
        t /= a.tiles_x;
        const int ty = t % a.tiles_y;
        const int b = t / a.tiles_y;
        const int y0 = ty * TH, x0 = tx * TW;
        float* bufA = lds + buf * T::BUF;
        float* bufB = bufA + T::COT * SA;
        const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.dz + (size_t)b * a.Cout * plane), 0, (int)(a.Cout * plane * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.x1 + (size_t)b * a.C1 * plane1), 0, (int)(a.C1 * plane1 * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.x2 ? a.x2 + (size_t)b * a.C2 * plane : a.x1), 0, (int)(a.C2 * plane * 4), 0x00020000);
        // per-lane byte offsets inside a channel plane for the PA / PB pieces of a row (same for every row)
        unsigned oz[T::PA], o1[T::PB], o2[T::PB];
#pragma unroll
        for (int i = 0; i < T::PA; ++i) {
            const int p = i * 64 + lane;
            const int oy = y0 + p / TW, ox = x0 + p % TW;
            oz[i] = (p < NPIX && oy < H && ox < W) ? (unsigned)(oy * W + ox) * 4u : kOOB;
        }
#pragma unroll
        for (int i = 0; i < T::PB; ++i) {
            const int p = i * 64 + lane;
            int gy = y0 + p / PW - HALO, gx = x0 + p % PW - HALO;
            bool ok = p < T::NPATCH;
            if (HALO) {
                ok = pad_coord(gy, H, a.pad_mode) && ok;
                ok = pad_coord(gx, W, a.pad_mode) && ok;
            }
            ok = ok && gy >= 0 && gx >= 0 && gy < H && gx < W;
            gy = min(max(gy, 0), H - 1);
            gx = min(max(gx, 0), W - 1);
            o2[i] = ok ? (unsigned)(gy * W + gx) * 4u : kOOB;
            o1[i] = ok ? (unsigned)((gy / a.up1) * a.W1 + gx / a.up1) * 4u : kOOB;
        }
        for (int c = wave; c < T::COT; c += NWAVES) {       // wave-uniform rows
            const int co = co0 + c;
            const unsigned so = (unsigned)min(co, a.Cout - 1) * pbz;
#pragma unroll
            for (int i = 0; i < T::PA; ++i) wg_dma4(rz, (lds_ptr_t)(bufA + c * SA + i * 64), co < a.Cout ? oz[i] : kOOB, so);
        }
        for (int c = wave; c < T::CIT; c += NWAVES) {
            const int ci = ci0 + c;
            const bool from1 = ci < a.C1;
            const unsigned so = from1 ? (unsigned)ci * pb1 : (unsigned)min(max(ci - a.C1, 0), max(a.C2 - 1, 0)) * pbz;
#pragma unroll
            for (int i = 0; i < T::PB; ++i) {
                const unsigned vo = ci < a.Cin ? (from1 ? o1[i] : o2[i]) : kOOB;
                if (from1) wg_dma4(r1, (lds_ptr_t)(bufB + c * SB + i * 64), vo, so);
                else wg_dma4(r2, (lds_ptr_t)(bufB + c * SB + i * 64), vo, so);
            }
        }
    };

    if (t_begin < t_end) stage(t_begin, 0);
    __syncthreads();

    for (int tile = t_begin; tile < t_end; ++tile) {
        const int buf = (tile - t_begin) & 1;
        if (tile + 1 < t_end) stage(tile + 1, buf ^ 1);
        const float* ldsA = lds + buf * T::BUF;
        const float* ldsB = ldsA + T::COT * SA;
        const float* pa = ldsA + (wm * MR * 16 + (lane & 15)) * SA + (lane >> 4);
        const float* pb = ldsB + (wn * NC * 16 + (lane & 15)) * SB + (lane >> 4);
        // K-steps of 4 pixels, fully unrolled (every LDS offset is an immediate) and software-pipelined one step deep: the
        // fragments of step q+1 are requested before the MFMAs of step q are issued and sched_barrier pins that order --
        // with 2 waves per SIMD an LDS round trip in front of every group of MFMAs was the main loss (59-77 TFLOP/s).
        constexpr int QS = NPIX / 4;
        float af[2][MR], bf[2][NC][TAPS];
        auto fetch = [&](int qs) {
            const int q = qs * 4, py = q / TW, px = q % TW, sl = qs & 1;
#pragma unroll
            for (int m = 0; m < MR; ++m) af[sl][m] = pa[m * 16 * SA + q];
#pragma unroll
            for (int n = 0; n < NC; ++n)
#pragma unroll
                for (int t = 0; t < TAPS; ++t) {
                    const int ky = TAPS == 9 ? t / 3 : 0, kx = TAPS == 9 ? t % 3 : 0;
                    bf[sl][n][t] = pb[n * 16 * SB + (py + ky) * PW + px + kx];
                }
        };
        fetch(0);
#pragma unroll
        for (int qs = 0; qs < QS; ++qs) {
            if (qs + 1 < QS) fetch(qs + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int n = 0; n < NC; ++n)
#pragma unroll
                for (int t = 0; t < TAPS; ++t)
#pragma unroll
                    for (int m = 0; m < MR; ++m)
                        acc[m][n][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[qs & 1][m], bf[qs & 1][n][t], acc[m][n][t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (a.want_bias && blockIdx.x == 0 && tid < T::COT) bsum += wg_row_sum<NPIX>(ldsA + tid * SA);
        __syncthreads();
    }

    // ---- write this block's partial: D row = out channel (lane>>4)*4+r, D col = input channel lane&15
    const size_t nw = (size_t)a.Cout * a.Cin * TAPS;
    float* out = a.partial + (size_t)split * (nw + a.Cout);
#pragma unroll
    for (int n = 0; n < NC; ++n) {
        const int ci = ci0 + (wn * NC + n) * 16 + (lane & 15);
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + (wm * MR + m) * 16 + (lane >> 4) * 4 + r;
                if (co < a.Cout && ci < a.Cin) {
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) out[((size_t)co * a.Cin + ci) * TAPS + t] = acc[m][n][t][r];
                }
            }
    }
    if (a.want_bias && blockIdx.x == 0 && tid < T::COT && co0 + tid < a.Cout) out[nw + co0 + tid] = bsum;
}

// ------------------------------------------------------------------------------------------------
// Winograd F(2x2,3x3) weight gradient.
//   forward (conv_wino_kernel):  Y = A^T [ sum_ci U (.) V ] A,  U = G g G^T,  V = B^T d B   per 2x2 output tile
//   =>  dU_xi[co,ci] = sum_tiles dM_xi[tile,co] * V_xi[tile,ci],  dM = A dY A^T (2x2 -> 4x4),   dg = G^T dU G
// In the transformed domain each of the 16 positions xi is an independent GEMM with K = tiles: 16 MFMAs per 4 tiles
// (= 16 pixels) and (co-tile, ci-tile) pair instead of the 36 of the direct form (4 K-steps x 9 taps).  A lane owns one
// channel (l & 15) and one tile of the K-step (l >> 4) for BOTH operands: it reads the tile's 2x2 dz values and the 4x4
// input patch from LDS at immediate offsets and transforms them in registers (12 + 32 adds).  Staging (LDS-DMA gather of
// dz rows and of the padded / upsampled / concatenated patch rows, double buffered across pixel tiles), the split over
// pixel tiles (wg_split_range) and the bias row sums (wg_row_sum) are those of conv_wgrad_kernel; partials are [split][16][Cout*Cin] (+ [Cout] bias) and
// wgrad_wino_reduce_kernel sums them and applies G^T . G.
// ------------------------------------------------------------------------------------------------
template <int TH, int TW, int MR, int NC, int WM, int WN>
struct WgradWinoTile {
    static constexpr int NT = WM * WN * 64;
    static constexpr int PH = TH + 2, PW = TW + 2;
    static constexpr int NPIX = TH * TW, NPATCH = PH * PW;
    static constexpr int COT = WM * MR * 16, CIT = WN * NC * 16;
    static constexpr int TXW = TW / 2, NT2 = (TH / 2) * TXW, KS = NT2 / 4;
    // row strides == 2 (mod 32), no rounding to whole DMA pieces: the last piece of a row is exec-masked
    static constexpr int SA = ((NPIX - 2 + 31) / 32) * 32 + 2;
    static constexpr int SB = ((NPATCH - 2 + 31) / 32) * 32 + 2;
    static constexpr int PA = (NPIX + 63) / 64, PB = (NPATCH + 63) / 64;
    static constexpr int BUF = COT * SA + CIT * SB;
    static constexpr int LDS_FLOATS = 2 * BUF;
    static_assert(TH % 2 == 0 && TW % 8 == 0, "whole 2x2 tiles; the four tiles of a K-step stay in one tile row");
    static_assert(NT2 % 4 == 0, "whole K-steps");
};

template <int TH, int TW, int MR, int NC, int WM, int WN>
__global__ __launch_bounds__(WM* WN * 64) void conv_wgrad_wino_kernel(const WgradKArgs a) {
    using T = WgradWinoTile<TH, TW, MR, NC, WM, WN>;
    constexpr int PW = T::PW, SA = T::SA, SB = T::SB, NPIX = T::NPIX;
    constexpr int NWAVES = WM * WN;
    constexpr unsigned kOOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int co0 = blockIdx.y * T::COT, ci0 = blockIdx.x * T::CIT;
    const int split = blockIdx.z;
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W, plane1 = (size_t)a.H1 * a.W1;
    const unsigned pbz = (unsigned)(plane * 4), pb1 = (unsigned)(plane1 * 4);

    f32x4 acc[16][MR][NC];
#pragma unroll
    for (int xi = 0; xi < 16; ++xi)
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) acc[xi][m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;

    int t_begin, t_end;
    wg_split_range(a, split, t_begin, t_end);

    auto stage = [&](int tile, int buf) {
        int t = tile;
        const int tx = t % a.tiles_x;
        t /= a.tiles_x;
        const int ty = t % a.tiles_y;
        const int b = t / a.tiles_y;
        const int y0 = ty * TH, x0 = tx * TW;
        float* bufA = lds + buf * T::BUF;
        float* bufB = bufA + T::COT * SA;
        const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.dz + (size_t)b * a.Cout * plane), 0, (int)(a.Cout * plane * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.x1 + (size_t)b * a.C1 * plane1), 0, (int)(a.C1 * plane1 * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(a.x2 ? a.x2 + (size_t)b * a.C2 * plane : a.x1), 0, (int)(a.C2 * plane * 4), 0x00020000);
        unsigned oz[T::PA], o1[T::PB], o2[T::PB];
#pragma unroll
        for (int i = 0; i < T::PA; ++i) {
            const int p = i * 64 + lane;
            const int oy = y0 + p / TW, ox = x0 + p % TW;
            oz[i] = (p < NPIX && oy < H && ox < W) ? (unsigned)(oy * W + ox) * 4u : kOOB;
        }
#pragma unroll
        for (int i = 0; i < T::PB; ++i) {
            const int p = i * 64 + lane;
            int gy = y0 + p / PW - 1, gx = x0 + p % PW - 1;
            bool ok = p < T::NPATCH;
            ok = pad_coord(gy, H, a.pad_mode) && ok;
            ok = pad_coord(gx, W, a.pad_mode) && ok;
            ok = ok && gy >= 0 && gx >= 0 && gy < H && gx < W;
            gy = min(max(gy, 0), H - 1);
            gx = min(max(gx, 0), W - 1);
            o2[i] = ok ? (unsigned)(gy * W + gx) * 4u : kOOB;
            o1[i] = ok ? (unsigned)((gy / a.up1) * a.W1 + gx / a.up1) * 4u : kOOB;
        }
        for (int c = wave; c < T::COT; c += NWAVES) {       // wave-uniform rows
            const int co = co0 + c;
            const unsigned so = (unsigned)min(co, a.Cout - 1) * pbz;
#pragma unroll
            for (int i = 0; i < T::PA; ++i)
                if (T::PA * 64 == NPIX || i * 64 + lane < NPIX)   // partial last piece: exec-masked
                    wg_dma4(rz, (lds_ptr_t)(bufA + c * SA + i * 64), co < a.Cout ? oz[i] : kOOB, so);
        }
        for (int c = wave; c < T::CIT; c += NWAVES) {
            const int ci = ci0 + c;
            const bool from1 = ci < a.C1;
            const unsigned so = from1 ? (unsigned)ci * pb1 : (unsigned)min(max(ci - a.C1, 0), max(a.C2 - 1, 0)) * pbz;
#pragma unroll
            for (int i = 0; i < T::PB; ++i) {
                const unsigned vo = ci < a.Cin ? (from1 ? o1[i] : o2[i]) : kOOB;
                if (T::PB * 64 == T::NPATCH || i * 64 + lane < T::NPATCH) {
                    if (from1) wg_dma4(r1, (lds_ptr_t)(bufB + c * SB + i * 64), vo, so);
                    else wg_dma4(r2, (lds_ptr_t)(bufB + c * SB + i * 64), vo, so);
                }
            }
        }
    };

    if (t_begin < t_end) stage(t_begin, 0);
    __syncthreads();

    for (int tile = t_begin; tile < t_end; ++tile) {
        const int buf = (tile - t_begin) & 1;
        if (tile + 1 < t_end) stage(tile + 1, buf ^ 1);
        const float* ldsA = lds + buf * T::BUF;
        const float* ldsB = ldsA + T::COT * SA;
        // lane = (channel l & 15, tile l >> 4 of the K-step): the tile's column offset 2 * (l >> 4) lives in the base pointers
        const float* pa = ldsA + (wm * MR * 16 + (lane & 15)) * SA + 2 * (lane >> 4);
        const float* pb = ldsB + (wn * NC * 16 + (lane & 15)) * SB + 2 * (lane >> 4);
        float dzr[2][MR][4], xr[2][NC][16];
        auto fetch = [&](int ks) {
            const int t0 = ks * 4, trow = t0 / T::TXW, tcol = t0 % T::TXW, sl = ks & 1;
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 2; ++c) dzr[sl][m][r * 2 + c] = pa[m * 16 * SA + (2 * trow + r) * TW + 2 * tcol + c];
#pragma unroll
            for (int n = 0; n < NC; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) xr[sl][n][r * 4 + c] = pb[n * 16 * SB + (2 * trow + r) * PW + 2 * tcol + c];
        };
        fetch(0);
#pragma unroll
        for (int ks = 0; ks < T::KS; ++ks) {
            const int sl = ks & 1;
            if (ks + 1 < T::KS) fetch(ks + 1);
            // dM = A dY A^T,  A = [[1,0],[1,1],[1,-1],[0,-1]]
            float dm[MR][16], v[NC][16];
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                const float d00 = dzr[sl][m][0], d01 = dzr[sl][m][1], d10 = dzr[sl][m][2], d11 = dzr[sl][m][3];
                const float t[4][2] = {{d00, d01}, {d00 + d10, d01 + d11}, {d00 - d10, d01 - d11}, {-d10, -d11}};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    dm[m][r * 4 + 0] = t[r][0];
                    dm[m][r * 4 + 1] = t[r][0] + t[r][1];
                    dm[m][r * 4 + 2] = t[r][0] - t[r][1];
                    dm[m][r * 4 + 3] = -t[r][1];
                }
            }
            // V = B^T d B (as in conv_wino_kernel)
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                float tr[16];
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    tr[0 * 4 + cc] = xr[sl][n][0 * 4 + cc] - xr[sl][n][2 * 4 + cc];
                    tr[1 * 4 + cc] = xr[sl][n][1 * 4 + cc] + xr[sl][n][2 * 4 + cc];
                    tr[2 * 4 + cc] = xr[sl][n][2 * 4 + cc] - xr[sl][n][1 * 4 + cc];
                    tr[3 * 4 + cc] = xr[sl][n][1 * 4 + cc] - xr[sl][n][3 * 4 + cc];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[n][r * 4 + 0] = tr[r * 4 + 0] - tr[r * 4 + 2];
                    v[n][r * 4 + 1] = tr[r * 4 + 1] + tr[r * 4 + 2];
                    v[n][r * 4 + 2] = tr[r * 4 + 2] - tr[r * 4 + 1];
                    v[n][r * 4 + 3] = tr[r * 4 + 1] - tr[r * 4 + 3];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int xi = 0; xi < 16; ++xi)
#pragma unroll
                for (int n = 0; n < NC; ++n)
#pragma unroll
                    for (int m = 0; m < MR; ++m)
                        acc[xi][m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(dm[m][xi], v[n][xi], acc[xi][m][n], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (a.want_bias && blockIdx.x == 0 && tid < T::COT) bsum += wg_row_sum<NPIX>(ldsA + tid * SA);
        __syncthreads();
    }

    // partial [split][16][Cout*Cin] (+ [Cout] bias sums): D row = out channel (lane>>4)*4+r, D col = input channel lane&15
    const size_t nwc = (size_t)a.Cout * a.Cin;
    float* out = a.partial + (size_t)split * (16 * nwc + a.Cout);
#pragma unroll
    for (int n = 0; n < NC; ++n) {
        const int ci = ci0 + (wn * NC + n) * 16 + (lane & 15);
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + (wm * MR + m) * 16 + (lane >> 4) * 4 + r;
                if (co < a.Cout && ci < a.Cin) {
#pragma unroll
                    for (int xi = 0; xi < 16; ++xi) out[(size_t)xi * nwc + (size_t)co * a.Cin + ci] = acc[xi][m][n][r];
                }
            }
    }
    if (a.want_bias && blockIdx.x == 0 && tid < T::COT && co0 + tid < a.Cout) out[16 * nwc + co0 + tid] = bsum;
}

// dg = G^T (sum over splits of dU) G per (co, ci); thread (w, xi) sums position xi of weight w over the splits, the block
// combines the 16 positions through LDS.  G = [[1,0,0],[1/2,1/2,1/2],[1/2,-1/2,1/2],[0,0,1]].
__global__ __launch_bounds__(1024) void wgrad_wino_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                                                 float* __restrict__ db, size_t nwc, int Cout, int nsplit) {
    // thread (w, g): weight w of the block's 64, split group g of 16 -- sums all 16 positions over the splits s == g (mod 16)
    // (16 independent accumulators = 16 loads in flight), the block then combines the groups through LDS (two passes of 8
    // positions keep it at 32 KB) and 9 x 64 threads apply G^T . G.
    __shared__ float red[16][8][64];
    __shared__ float u[16][64];
    const int w = threadIdx.x & 63, g = threadIdx.x >> 6;
    const size_t stride = 16 * nwc + Cout;
    const size_t i = (size_t)blockIdx.x * 64 + w;
    float acc[16];
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) acc[xi] = 0.f;
    if (i < nwc) {
        for (int s = g; s < nsplit; s += 16) {
            const float* p = partial + (size_t)s * stride + i;
#pragma unroll
            for (int xi = 0; xi < 16; ++xi) acc[xi] += p[(size_t)xi * nwc];
        }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int k = 0; k < 8; ++k) red[g][k][w] = acc[half * 8 + k];
        __syncthreads();
        if (g < 8) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += red[q][g][w];
            u[half * 8 + g][w] = t;
        }
        __syncthreads();
    }
    if (g < 9 && i < nwc) {
        const float G[4][3] = {{1.f, 0.f, 0.f}, {0.5f, 0.5f, 0.5f}, {0.5f, -0.5f, 0.5f}, {0.f, 0.f, 1.f}};
        const int ky = g / 3, kx = g % 3;
        float t = 0.f;
#pragma unroll
        for (int pa_ = 0; pa_ < 4; ++pa_)
#pragma unroll
            for (int pb_ = 0; pb_ < 4; ++pb_) t += G[pa_][ky] * G[pb_][kx] * u[pa_ * 4 + pb_][w];
        dw[i * 9 + g] = t;
    }
    if (db && blockIdx.x == gridDim.x - 1) {
        // bias: 64 channels per pass, the 16 groups stride over the splits (a serial loop over up to 128 partials per
        // channel was a 40 us chain of dependent loads)
        __syncthreads();
        for (int c0 = 0; c0 < Cout; c0 += 64) {
            const int c = c0 + w;
            float t = 0.f;
            if (c < Cout)
                for (int s = g; s < nsplit; s += 16) t += partial[(size_t)s * stride + 16 * nwc + c];
            red[g][0][w] = t;
            __syncthreads();
            if (g == 0 && c < Cout) {
                float r = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) r += red[q][0][w];
                db[c] = r;
            }
            __syncthreads();
        }
    }
}

// dw[i] (and db) = sum over the split partials.  Block = 64 outputs x 16 split groups; the groups are combined
// through LDS, so even a 1024-element weight with hundreds of partials is a handful of dependent loads per thread.
__global__ __launch_bounds__(1024) void wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                                            float* __restrict__ db, size_t nw, int Cout, int nsplit) {
    __shared__ float red[16][64];
    const int w = threadIdx.x & 63, g = threadIdx.x >> 6;
    const size_t n = nw + Cout;
    const size_t i = (size_t)blockIdx.x * 64 + w;
    float v = 0.f;
    if (i < n) {
        int s = g;
        for (; s + 48 < nsplit; s += 64) {   // four independent loads in flight per trip, fixed summation order
            const float p0 = partial[(size_t)s * n + i], p1 = partial[(size_t)(s + 16) * n + i];
            const float p2 = partial[(size_t)(s + 32) * n + i], p3 = partial[(size_t)(s + 48) * n + i];
            v = (((v + p0) + p1) + p2) + p3;
        }
        for (; s < nsplit; s += 16) v += partial[(size_t)s * n + i];
    }
    red[g][w] = v;
    __syncthreads();
    if (g == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][w];
        if (i < nw) dw[i] = t;
        else if (db) db[i - nw] = t;
    }
}

// Weight gradient of the wavelet heads' last convolution (Cout <= 4: an MFMA tile would be > 75 % padding):
//   dW[co,ci,t] = sum_{b,y,x} dz[b,co,y,x] * pad(x)[b,ci,y+ky,x+kx]
// One block per (input channel, image, row slab).  A thread owns one column of one of `nseg` row segments of the
// slab and walks down it with the 3x3 window in registers (3 new loads of x + COUT of dz per pixel), 9*COUT
// accumulators; then a wavefront shuffle + LDS reduction.  Channel-0 blocks also produce the bias partial sums.
// Partials use the same [split][Cout*Cin*9 + Cout] layout as the MFMA path, so wgrad_reduce_kernel finishes both.
template <int COUT>
__global__ __launch_bounds__(256) void conv_wgrad_smallco_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                                 float* __restrict__ partial, int C, int H, int W,
                                                                 int pad_mode, int spi, int nseg, int want_bias) {
    const int ci = blockIdx.x, split = blockIdx.y;
    const int b = split / spi, sl = split - b * spi;
    const int rps = (H + spi - 1) / spi;
    const int r0 = sl * rps, r1 = min(H, r0 + rps);
    const int rseg = (max(r1 - r0, 0) + nseg - 1) / nseg;
    const size_t plane = (size_t)H * W;
    const float* xp = x + ((size_t)b * C + ci) * plane;
    const float* gp = dz + (size_t)b * COUT * plane;
    float acc[COUT][9], bs[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
        bs[co] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[co][t] = 0.f;
    }
    for (int item = threadIdx.x; item < W * nseg; item += 256) {
        const int seg = item / W, xx = item - seg * W;
        const int y0 = r0 + seg * rseg, y1 = min(r1, y0 + rseg);
        if (y0 >= y1) continue;
        int cx[3];
        bool okx[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            cx[d] = xx + d - 1;
            okx[d] = pad_coord(cx[d], W, pad_mode);
            cx[d] = min(max(cx[d], 0), W - 1);
        }
        auto load_row = [&](int yy, float* out) {
            const bool oky = pad_coord(yy, H, pad_mode);
            const float* rp = xp + (size_t)min(max(yy, 0), H - 1) * W;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float v = rp[cx[d]];
                out[d] = (oky && okx[d]) ? v : 0.f;
            }
        };
        float win[9];
        load_row(y0 - 1, win);
        load_row(y0, win + 3);
#pragma unroll 4
        for (int y = y0; y < y1; ++y) {   // unrolled: the next rows' loads are issued ahead of this row's FMAs
            load_row(y + 1, win + 6);
#pragma unroll
            for (int co = 0; co < COUT; ++co) {
                const float g = gp[co * plane + (size_t)y * W + xx];
                bs[co] += g;
#pragma unroll
                for (int t = 0; t < 9; ++t) acc[co][t] = fmaf(g, win[t], acc[co][t]);
            }
#pragma unroll
            for (int t = 0; t < 6; ++t) win[t] = win[t + 3];
        }
    }
    __shared__ float red[4][COUT * 10];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
#pragma unroll
        for (int t = 0; t < 10; ++t) {
            float s = t < 9 ? acc[co][t] : bs[co];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0) red[wave][co * 10 + t] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < COUT * 10) {
        const float s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        const int co = threadIdx.x / 10, t = threadIdx.x % 10;
        const size_t nw = (size_t)COUT * C * 9;
        float* out = partial + (size_t)split * (nw + COUT);
        if (t < 9) out[((size_t)co * C + ci) * 9 + t] = s;
        else if (want_bias && ci == 0) out[nw + co] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// host side: switches, configuration tables, planner, launcher
// ------------------------------------------------------------------------------------------------
// Every WMD_WGRAD_* environment switch.  Development switches, read on every call (tests and tools set them between calls),
// except the split cap, which is read at the first call and fixed for the life of the process.
struct WgradSwitches {
    int cfg;          // WMD_WGRAD_CFG=<1-based index into kWCfgs> forces a direct entry (-1: none; an entry of the other tap count is ignored)
    int wino_cfg;     // WMD_WGRAD_WINO_CFG=<1-based index into kWWCfgs> forces a Winograd entry (wmd_conv_wgrad_args.tune_cfg wins)
    int nsplit;       // WMD_WGRAD_NSPLIT=<n> forces the pixel split (wmd_conv_wgrad_args.tune_nsplit wins)
    bool wino;        // WMD_WGRAD_WINO=0 switches the Winograd entries off
    bool smallco;     // WMD_WGRAD_SMALLCO=1: the heads' Cout <= 4 filters run the VALU column-walk kernel
    long nsplit_cap;  // WMD_WGRAD_NSPLIT_CAP: most partial slices of a Winograd plan (128 until round 4: single-slab layers -- Cout = 32 -- then ran 256 blocks on 512 slots: L14 242 -> 209 us)
};
static WgradSwitches wgrad_switches() {
    auto num = [](const char* v, int dflt) { return v ? atoi(v) : dflt; };
    static const int cap = num(getenv("WMD_WGRAD_NSPLIT_CAP"), 0);
    WgradSwitches s;
    s.cfg = num(getenv("WMD_WGRAD_CFG"), 0) - 1;
    s.wino_cfg = num(getenv("WMD_WGRAD_WINO_CFG"), 0) - 1;
    s.nsplit = num(getenv("WMD_WGRAD_NSPLIT"), 0);
    s.wino = num(getenv("WMD_WGRAD_WINO"), 1) != 0;
    s.smallco = num(getenv("WMD_WGRAD_SMALLCO"), 0) == 1;
    s.nsplit_cap = cap > 0 ? cap : 256;
    return s;
}

enum class WgradFamily {
    Direct3x3,   // conv_wgrad_kernel, TAPS = 9
    Direct1x1,   // conv_wgrad_kernel, TAPS = 1: the pixel domain is flattened to 1 x HW
    Wino16,      // conv_wgrad_wino_kernel: F(2x2,3x3) on 16x16x4 MFMAs
    Wino32,      // conv_wgrad_wino32_kernel (wmd_conv_wgrad32.hip): F(2x2,3x3) on 32x32x2 MFMAs
};
static bool fam_wino(WgradFamily f) { return f == WgradFamily::Wino16 || f == WgradFamily::Wino32; }
static int fam_taps(WgradFamily f) { return f == WgradFamily::Direct1x1 ? 1 : 9; }   // filter taps served

struct WgradCfg {
    WgradFamily family;
    int TH, TW;      // pixel tile
    int cot, cit;    // out / in channels per block
    int bpc;         // blocks that share a CU (the pixel split aims at this many rounds-free blocks per CU)
    double eff;      // cost-model factor: two ci / co tiles per wave amortise the Winograd transforms (0.93); 32x32x2 runs ~2x the rate (0.5)
    void (*launch)(const WgradKArgs&, dim3, hipStream_t);
    const char* name;
};

template <int TH, int TW, int MR, int NC, int WM, int WN, int TAPS>
static void launch_wgrad(const WgradKArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((conv_wgrad_kernel<TH, TW, MR, NC, WM, WN, TAPS>), grid, dim3(WM * WN * 64), 0, s, a);
}
#define WMD_WCFG(TH, TW, MR, NC, WM, WN, TAPS)                                                                              \
    WgradCfg {                                                                                                              \
        TAPS == 9 ? WgradFamily::Direct3x3 : WgradFamily::Direct1x1, TH, TW, (WM) * (MR) * 16, (WN) * (NC) * 16, 2, 1.0,    \
            &launch_wgrad<TH, TW, MR, NC, WM, WN, TAPS>,                                                                    \
            "conv_wgrad_kernel<" #TH "," #TW "," #MR "," #NC "," #WM "," #WN "," #TAPS ">"                                  \
    }

// the direct entries; WMD_WGRAD_CFG counts them from 1
static const WgradCfg kWCfgs[] = {
    WMD_WCFG(2, 32, 1, 1, 4, 1, 9),   // co64 x ci16, 64-pixel tiles
    WMD_WCFG(2, 32, 1, 1, 2, 2, 9),   // co32 x ci32
    WMD_WCFG(1, 40, 1, 1, 4, 1, 9),   // 40-wide rows: one row per tile keeps the double buffer at 50 KB (3 blocks / CU;
    WMD_WCFG(1, 40, 1, 1, 2, 2, 9),   //   the 2 x 40 tile needs 91 KB = 1 block / CU and ran at 50 instead of 76 TFLOP/s)
    WMD_WCFG(2, 20, 1, 1, 4, 1, 9),   // 20-wide rows (coarsest 640-wide level, NYUv2 15x20)
    WMD_WCFG(2, 20, 1, 1, 2, 2, 9),
    WMD_WCFG(1, 32, 2, 1, 2, 2, 9),   // co64 x ci32, MR = 2: 18 MFMAs per 2 + 9 fragment reads (67 KB: 2 blocks / CU)
    WMD_WCFG(2, 32, 2, 1, 2, 2, 9),   // co64 x ci32, 64-pixel tiles
    WMD_WCFG(1, 32, 2, 2, 2, 1, 9),   // co64 x ci32 in 2 waves: 36 MFMAs per 4 + 18 reads
    WMD_WCFG(1, 40, 2, 1, 2, 2, 9),   // 40-wide rows
    WMD_WCFG(1, 32, 1, 1, 1, 4, 9),   // co16 x ci64: the heads' Cout <= 4 filters on the matrix pipe (3/16 of the rows used)
    WMD_WCFG(1, 40, 1, 1, 1, 4, 9),
    WMD_WCFG(1, 64, 1, 4, 4, 1, 1),   // 1x1: co64 x ci64 over 64 flattened pixels
    WMD_WCFG(1, 64, 1, 2, 2, 2, 1),   // 1x1: co32 x ci64
};
constexpr int kNumWCfgs = sizeof(kWCfgs) / sizeof(kWCfgs[0]);

template <int TH, int TW, int MR, int NC, int WM, int WN>
static void launch_wgrad_wino(const WgradKArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((conv_wgrad_wino_kernel<TH, TW, MR, NC, WM, WN>), grid, dim3(WM * WN * 64), 0, s, a);
}
#define WMD_WWCFG(TH, TW, MR, NC, WM, WN)                                                                       \
    WgradCfg {                                                                                                  \
        WgradFamily::Wino16, TH, TW, (WM) * (MR) * 16, (WN) * (NC) * 16, 2, (MR) * (NC) > 1 ? 0.93 : 1.0,       \
            &launch_wgrad_wino<TH, TW, MR, NC, WM, WN>,                                                         \
            "conv_wgrad_wino_kernel<" #TH "," #TW "," #MR "," #NC "," #WM "," #WN ">"                           \
    }
// conv_wgrad_wino32_kernel (wmd_conv_wgrad32.hip): WCO x WCI slabs of 32 out / 32 in channels per block
#define WMD_WG32_INST(TH, TW, WCO, WCI)                                                                               \
    WgradCfg{WgradFamily::Wino32, TH, TW, (WCO) * 32, (WCI) * 32, (WCO) * (WCI) >= 4 ? 1 : 2, 0.5,                    \
             &launch_wgrad_wino32<TH, TW, WCO, WCI>, "conv_wgrad_wino32_kernel<" #TH "," #TW "," #WCO "," #WCI ">"},
// the Winograd entries; wmd_conv_wgrad_args.tune_cfg = k, WMD_WGRAD_WINO_CFG = k and wmd_conv_wgrad_config_name(k - 1) name entry k - 1
static const WgradCfg kWWCfgs[] = {
    WMD_WWCFG(2, 32, 1, 1, 4, 1),   // co64 x ci16, 64-pixel tiles (55 KB: 2 blocks / CU)
    WMD_WWCFG(2, 32, 1, 1, 2, 2),   // co32 x ci32
    WMD_WWCFG(2, 32, 1, 2, 4, 1),   // co64 x ci32: two ci tiles per wave share the dz transform (75 KB)
    WMD_WWCFG(2, 32, 2, 1, 2, 2),   // co64 x ci32 in 4 waves
    WMD_WWCFG(2, 32, 1, 2, 2, 1),   // co32 x ci32 in 2 waves
    WMD_WWCFG(2, 40, 1, 1, 4, 1),   // 40-wide rows (W = 40 / 80 / 160 / 320)
    WMD_WWCFG(2, 40, 1, 1, 2, 2),
    WMD_WWCFG(4, 16, 1, 1, 4, 1),   // 16-wide tiles: narrow maps
    WMD_WWCFG(4, 16, 1, 2, 4, 1),
    WMD_WWCFG(2, 32, 1, 1, 1, 4),   // co16 x ci64: the heads' Cout <= 4 filters (3/16 of the MFMA rows carry data)
    WMD_WWCFG(2, 40, 1, 1, 1, 4),
    WMD_WWCFG(2, 32, 1, 2, 1, 2),   // co16 x ci64 in 2 waves
#include "wmd_conv_wgrad32_table.inc"
};
constexpr int kNumWWCfgs = sizeof(kWWCfgs) / sizeof(kWWCfgs[0]);

struct WgradPlan {
    const WgradCfg* cfg;    // nullptr: conv_wgrad_smallco_kernel
    int H, W;               // the pixel domain the kernel sees (1 x HW for a 1x1 filter)
    int tiles_x, tiles_y, ntiles, nsplit;
    int spi, nseg;          // conv_wgrad_smallco_kernel: row slabs per image (nsplit = B * spi), row segments per slab walked concurrently by one block
    dim3 grid;
    size_t slice_floats;    // one partial slice: the weights (16 positions of each in the Winograd domain), then Cout bias sums
};

// The cheapest of tab's entries that serve the layer, or entry `force` alone (< 0: none forced).
static bool plan_wgrad_mfma(const wmd_conv_wgrad_args* g, const WgradSwitches& sw, const WgradCfg* tab, int n, int force, long ns_cap,
                            WgradPlan* p) {
    const int taps = g->ksize == 3 ? 9 : 1;
    const int Cin = g->C1 + g->C2;
    const int H = taps == 9 ? g->H : 1, W = taps == 9 ? g->W : g->H * g->W;
    const int pinned = force >= 0 && force < n && fam_taps(tab[force].family) == taps ? force : -1;
    double best = 1e300;
    bool found = false;
    for (int i = 0; i < n; ++i) {
        const WgradCfg& c = tab[i];
        if (fam_taps(c.family) != taps || (pinned >= 0 && i != pinned)) continue;
        if (force < 0 && c.cot == 16 && g->Cout > 16) continue;   // 16-row out-channel tiles are for the heads only
        const int tx = (W + c.TW - 1) / c.TW, ty = (H + c.TH - 1) / c.TH;
        const int gx = (Cin + c.cit - 1) / c.cit, gy = (g->Cout + c.cot - 1) / c.cot;
        const long ntiles = (long)g->B * tx * ty;
        // padded MACs: every block sweeps all pixel tiles of its split.  The Winograd form is for the 3x3 layers whose width
        // fills a tile row reasonably; everything else (20-wide maps, tiny maps) stays on the direct kernel
        const double pix_waste = (double)tx * c.TW * ty * c.TH / ((double)H * W);
        if (fam_wino(c.family) && force < 0 && pix_waste > 1.6) continue;
        const double waste = ((double)gx * c.cit / Cin) * ((double)gy * c.cot / g->Cout) * pix_waste;
        // ~bpc blocks per CU in flight, at least 4 pixel tiles per block (prologue amortisation), at most ns_cap partials
        long nsplit = std::max<long>(1, ((long)c.bpc * kNumCU + (long)gx * gy - 1) / ((long)gx * gy));
        nsplit = std::min<long>(nsplit, std::max<long>(1, ntiles / 4));
        nsplit = std::min<long>(nsplit, ns_cap);
        if (sw.nsplit > 0) nsplit = std::min<long>(sw.nsplit, std::max<long>(1, ntiles));
        if (g->tune_nsplit > 0) nsplit = std::min<long>(g->tune_nsplit, std::max<long>(1, ntiles));
        const double rounds = std::ceil((double)gx * gy * nsplit / ((double)c.bpc * kNumCU));
        const double cost = c.eff * waste * rounds * (double)c.bpc * kNumCU / ((double)gx * gy * nsplit);
        if (cost < best) {
            best = cost;
            found = true;
            *p = WgradPlan{&c, H, W, tx, ty, (int)ntiles, (int)nsplit, 0, 0, dim3((unsigned)gx, (unsigned)gy, (unsigned)nsplit),
                           (size_t)g->Cout * Cin * (fam_wino(c.family) ? 16 : taps) + g->Cout};
        }
    }
    return found;
}

// conv_wgrad_smallco_kernel's plan
static void plan_wgrad_smallco(const wmd_conv_wgrad_args* g, WgradPlan* p) {
    // ~2 blocks per CU over (channels x images x slabs) (measured: 1 -> 0.59, 2 -> 0.46, 4 -> 0.53, 8 -> 0.57 ms per step:
    // more slabs = more window prologues and partials), slabs of at least 8 rows
    long spi = (2L * kNumCU + (long)g->C1 * g->B - 1) / ((long)g->C1 * g->B);
    spi = std::max<long>(1, std::min<long>(spi, std::max(1, g->H / 8)));
    const int rps = (g->H + (int)spi - 1) / (int)spi;
    // segments: fill the 256 threads with whole columns, but keep the 2-row window prologue amortised
    double best = -1.0;
    int nseg = 1;
    for (int n = 1; n <= std::min(8, rps); ++n) {
        const int items = g->W * n, passes = (items + 255) / 256, rseg = (rps + n - 1) / n;
        const double score = (double)items / (passes * 256.0) * rseg / (rseg + 2.0);
        if (score > best) { best = score; nseg = n; }
    }
    const int nsplit = g->B * (int)spi;
    *p = WgradPlan{nullptr, g->H, g->W, 1, (int)spi, nsplit, nsplit, (int)spi, nseg, dim3(g->C1, nsplit),
                   (size_t)g->Cout * g->C1 * 9 + g->Cout};
}

// tune_cfg names a configuration that cannot run: an index past the Winograd table, below -1, or a Winograd entry for a
// 1x1 filter.  Refused (WMD_ERR_UNSUPPORTED), never served by another kernel than the one asked for.
static bool wgrad_forced_cfg_invalid(const wmd_conv_wgrad_args* g) {
    return g->tune_cfg < -1 || g->tune_cfg > kNumWWCfgs || (g->tune_cfg > 0 && g->ksize != 3);
}

// The one plan behind the workspace query and the launch.  WMD_WGRAD_SMALLCO=1 sends the heads' Cout <= 4 filters to the VALU
// column-walk kernel (round 1; default: the MFMA kernels with 16-row out-channel tiles -- 3/16 of the rows used, but the
// reduction over pixels runs on the matrix pipe and dz is read once per 64 input channels instead of once per channel).
// Otherwise a Winograd entry when the family is allowed (3x3, not switched off, tune_cfg >= 0: -1 asks for the direct kernel;
// a WMD_WGRAD_WINO_CFG past the table falls through) and one survives its filters, else a direct entry.
static bool plan_wgrad(const wmd_conv_wgrad_args* g, WgradPlan* p) {
    const WgradSwitches sw = wgrad_switches();
    if (sw.smallco && g->Cout <= 4 && g->ksize == 3 && g->up1 == 1 && g->C2 == 0) {
        plan_wgrad_smallco(g, p);
        return true;
    }
    const int wforce = g->tune_cfg > 0 ? g->tune_cfg - 1 : sw.wino_cfg;
    if (g->ksize == 3 && sw.wino && g->tune_cfg >= 0 && wforce < kNumWWCfgs &&
        plan_wgrad_mfma(g, sw, kWWCfgs, kNumWWCfgs, wforce, sw.nsplit_cap, p))
        return true;
    return plan_wgrad_mfma(g, sw, kWCfgs, kNumWCfgs, sw.cfg, 256, p);
}

static WgradKArgs wgrad_kargs(const wmd_conv_wgrad_args* g, const WgradPlan& p) {
    WgradKArgs a;
    a.x1 = g->x1;
    a.x2 = g->x2;
    a.dz = g->dz;
    a.partial = g->workspace;
    a.B = g->B;
    a.H = p.H;
    a.W = p.W;
    a.up1 = g->ksize == 3 ? g->up1 : 1;
    a.H1 = p.H / a.up1;
    a.W1 = p.W / a.up1;
    a.C1 = g->C1;
    a.C2 = g->C2;
    a.Cin = g->C1 + g->C2;
    a.Cout = g->Cout;
    a.pad_mode = g->pad_mode;
    a.tiles_x = p.tiles_x;
    a.tiles_y = p.tiles_y;
    a.ntiles = p.ntiles;
    a.nsplit = p.nsplit;
    a.want_bias = g->dbias != nullptr;
    return a;
}

static void launch_wgrad_smallco(const WgradKArgs& a, const WgradPlan& p, hipStream_t s) {
    static void (*const kernels[4])(const float*, const float*, float*, int, int, int, int, int, int, int) = {
        conv_wgrad_smallco_kernel<1>, conv_wgrad_smallco_kernel<2>, conv_wgrad_smallco_kernel<3>, conv_wgrad_smallco_kernel<4>};
    hipLaunchKernelGGL(kernels[a.Cout - 1], p.grid, dim3(256), 0, s, a.x1, a.dz, a.partial, a.C1, a.H, a.W, a.pad_mode, p.spi, p.nseg,
                       a.want_bias);
}

}  // namespace wmd

using namespace wmd;

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int wmd_conv_wgrad_num_configs(void) { return kNumWWCfgs; }
extern "C" const char* wmd_conv_wgrad_config_name(int index) { return (index >= 0 && index < kNumWWCfgs) ? kWWCfgs[index].name : ""; }

extern "C" size_t wmd_conv_wgrad_workspace_floats(const wmd_conv_wgrad_args* g) {
    WgradPlan p;
    if (!g || g->B <= 0 || g->Cout <= 0 || wgrad_forced_cfg_invalid(g) || !plan_wgrad(g, &p)) return 0;
    return (size_t)p.nsplit * p.slice_floats;
}

extern "C" int wmd_conv_wgrad(const wmd_conv_wgrad_args* g, void* stream) {
    if (!g) return fail(WMD_ERR_BAD_ARG, "wmd_conv_wgrad: null args");
    if (!g->x1 || !g->dz || !g->dw) return fail(WMD_ERR_BAD_ARG, "wmd_conv_wgrad: null tensor pointer");
    if (g->C2 > 0 && !g->x2) return fail(WMD_ERR_BAD_ARG, "wmd_conv_wgrad: C2=%d but x2 is null", g->C2);
    int st = conv_check_problem(g->B, g->H, g->W, g->C1, g->up1, g->C2, g->Cout, g->ksize, g->pad_mode, WMD_ACT_NONE, "wmd_conv_wgrad");
    if (st) return st;
    if (g->ksize == 1 && g->up1 == 2) return fail(WMD_ERR_UNSUPPORTED, "wmd_conv_wgrad: 1x1 with upsampled input");
    if (wgrad_forced_cfg_invalid(g))
        return fail(WMD_ERR_UNSUPPORTED, "wmd_conv_wgrad: tune_cfg=%d cannot run (%d Winograd entries, 3x3 only; ksize=%d)", g->tune_cfg,
                    kNumWWCfgs, g->ksize);
    if ((double)std::max(g->C1, std::max(g->C2, g->Cout)) * g->H * g->W * 4 > 2147483647.0)
        return fail(WMD_ERR_UNSUPPORTED, "wmd_conv_wgrad: a per-image tensor slice exceeds 2 GiB");
    WgradPlan p;
    if (!plan_wgrad(g, &p)) return fail(WMD_ERR_UNSUPPORTED, "wmd_conv_wgrad: no kernel configuration");
    const size_t need = (size_t)p.nsplit * p.slice_floats;
    if (!g->workspace || g->workspace_floats < need)
        return fail(WMD_ERR_WORKSPACE, "wmd_conv_wgrad: workspace %zu < %zu floats", g->workspace_floats, need);
    const WgradKArgs a = wgrad_kargs(g, p);
    const bool wino = p.cfg && fam_wino(p.cfg->family);
    hipStream_t s = (hipStream_t)stream;
    const int taps = g->ksize == 3 ? 9 : 1;
    const size_t nwc = (size_t)a.Cout * a.Cin, nw = nwc * taps;
    const double pix = (double)g->B * g->H * g->W;
    {
        // (the VALU kernel's figures leave the weights out of the traffic, as they always have)
        ProfScope prof(p.cfg ? p.cfg->name : "conv_wgrad_smallco_kernel", 2.0 * a.Cin * taps * a.Cout * pix,
                       4.0 * (pix * (a.Cin + a.Cout) + (p.cfg ? (double)nw : 0.0)), s);
        if (p.cfg) p.cfg->launch(a, p.grid, s);
        else launch_wgrad_smallco(a, p, s);
    }
    st = check_launch(!p.cfg ? "conv_wgrad_smallco_kernel" : wino ? "conv_wgrad_wino_kernel" : "conv_wgrad_kernel");
    if (st) return st;
    if (wino) {   // sums the 16 positions over the slices and applies G^T . G
        ProfScope prof("wgrad_wino_reduce_kernel", 16.0 * nwc * p.nsplit, 4.0 * 16 * nwc * (p.nsplit + 1), s);
        hipLaunchKernelGGL(wgrad_wino_reduce_kernel, dim3((unsigned)((nwc + 63) / 64)), dim3(1024), 0, s, g->workspace, g->dw, g->dbias,
                           nwc, g->Cout, p.nsplit);
        return check_launch("wgrad_wino_reduce_kernel");
    }
    ProfScope prof("wgrad_reduce_kernel", (double)nw * p.nsplit, 4.0 * nw * (p.nsplit + 1), s);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((nw + g->Cout + 63) / 64)), dim3(1024), 0, s, g->workspace, g->dw, g->dbias,
                       nw, g->Cout, p.nsplit);
    return check_launch("wgrad_reduce_kernel");
}
