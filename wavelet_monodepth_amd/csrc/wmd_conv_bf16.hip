// Opt-in reduced-precision trunk convolution: direct implicit-GEMM 3x3 on v_mfma_f32_32x32x16_bf16 (include/wmd.h,
// wmd_conv_bf16_fwd).  Operands are rounded to bf16 on the way into LDS (TERMS = 1) or split into a bf16 head and a bf16
// tail (TERMS = 3: xh*wh + xh*wl + xl*wh, the tail x tail product is dropped); products are exact in fp32 and the
// accumulator, bias, activation and the stored result are fp32.  Same fusion as conv_fwd_kernel: nearest x2 upsample of x1,
// channel concat with x2, reflect / zero border addressing, bias + activation in the epilogue.
//
// Block = 256 threads = 4 waves.  The block owns TH x TW output pixels (= 4 * NR groups of 32 pixels, row-major over the
// tile) and MR slabs of 32 output channels; every wave owns NR pixel groups and all MR slabs, i.e. MR x NR accumulator
// tiles of the 32x32x16 MFMA with the output channel on the MFMA row (A = weights) and the pixel on the MFMA column
// (B = activations): a lane's 16 results are 16 output channels of one pixel, 32 adjacent lanes are 32 adjacent pixels.
//
// The reduction runs over chunks of 16 input channels (one MFMA k-step per tap).  Per chunk the block stages
//   - the (TH+2) x (TW+2) halo tile of the 16 channels: read as fp32, converted in registers, written to LDS as bf16 with the
//     channel innermost -- 32 bytes per halo pixel and plane (head, tail), in two 16-byte halves of 8 channels.  A lane's B
//     fragment (8 consecutive channels of one pixel) is one ds_read_b128 and the nine taps are nine pixel offsets into the
//     same image.  The two halves of a pixel trade places when bit 3 of the halo pixel index is set, which makes the 16-lane
//     groups a ds_read_b128 is served in (32 consecutive pixels, lane halves 16 bytes apart) touch 16 different 16-byte slots;
//   - the chunk's weights, already in fragment order in the packed image (1 KiB per slab, tap and plane): copied as is.
// Global loads of chunk c + 1 are issued before the MFMAs of chunk c and land in registers (LDS-DMA cannot convert).
#include <algorithm>
#include <string.h>
#include "wmd_conv_common.h"

namespace wmd {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

struct Bf16KArgs {
    const float* x1;
    const float* x2;
    const u32x4* wp;      // packed image in 16-byte pieces: [plane][Cout/32][Cin/16][tap][lane]
    const float* bias;
    float* y;             // final output (ksplit == 1) or partial sums [ksplit][B,Cout,H,W]
    int B, H, W, H1, W1, C1, C2, Cout, up1, pad_mode, act;
    float slope;
    int tiles_x, tiles_y, cob;   // pixel tiles per frame, blocks of MR slabs per pixel tile
    int nchunks, ksplit, cps;    // 16-channel chunks, K slices, chunks per slice
    int plane_pieces;            // 16-byte pieces of one plane of the weight image
};

constexpr int kThreads = 256;
constexpr int kTapPieces = 64;              // one fragment: 64 lanes x 16 bytes
constexpr int kChunkPieces = 9 * kTapPieces;   // one slab, one chunk, one plane

template <int TH, int TW, int MR, int NR, int TERMS>
struct B16Tile {
    static constexpr int PL = TERMS == 3 ? 2 : 1;
    static constexpr int HWID = TW + 2, HP = (TH + 2) * HWID;     // halo tile
    static constexpr int NIT = (2 * HP + kThreads - 1) / kThreads;   // (pixel, channel half) items per thread
    static constexpr int WPIECES = MR * PL * kChunkPieces;
    static constexpr int NWP = (WPIECES + kThreads - 1) / kThreads;
    static constexpr int W_BYTES = WPIECES * 16;
    static constexpr int X_PLANE_BYTES = HP * 32;
    static constexpr int LDS_BYTES = W_BYTES + PL * X_PLANE_BYTES;
    static_assert(TERMS == 1 || TERMS == 3, "one product or the three-product split");
    static_assert(TH * TW == 4 * NR * 32, "four waves x NR groups of 32 pixels");
    static_assert((TW & (TW - 1)) == 0 && TW <= 32, "a 32-pixel group is whole tile rows");
    static_assert(LDS_BYTES <= 64 * 1024, "two blocks per CU");
};

// byte offset of the 16-byte half `h` (channels 8h .. 8h+7) of halo pixel `pix` inside one plane of the LDS image
__device__ __forceinline__ int x_lds_off(int pix, int h) { return ((pix << 1) + (h ^ ((pix >> 3) & 1))) << 4; }

__device__ __forceinline__ float epi_act(float v, int act, float slope) {
    return act == WMD_ACT_ELU ? w32_act<WMD_ACT_ELU>(v, slope) : act == WMD_ACT_LEAKY ? w32_act<WMD_ACT_LEAKY>(v, slope)
         : act == WMD_ACT_SIGMOID ? w32_act<WMD_ACT_SIGMOID>(v, slope) : v;
}

template <int TH, int TW, int MR, int NR, int TERMS>
__global__ __launch_bounds__(kThreads) void conv_bf16_kernel(const Bf16KArgs a) {
    using T = B16Tile<TH, TW, MR, NR, TERMS>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[T::LDS_BYTES];
    unsigned char* const ws = smem;
    unsigned char* const xs = smem + T::W_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = blockIdx.x;
    const int cob_i = bid % a.cob;
    bid /= a.cob;
    const int tx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const int ty = bid % a.tiles_y, b = bid / a.tiles_y;
    const int ks = blockIdx.y;
    const int y0 = ty * TH, x0 = tx * TW, cot0 = cob_i * MR;
    const int c_begin = ks * a.cps, c_end = min(a.nchunks, c_begin + a.cps);
    const int H = a.H, W = a.W;
    const int plane1 = a.H1 * a.W1, plane2 = H * W;

    // this thread's staging items: source offsets inside a channel plane (-1: the position reads zero), LDS destination
    int off1[T::NIT], off2[T::NIT], xdst[T::NIT], xch[T::NIT];
#pragma unroll
    for (int i = 0; i < T::NIT; ++i) {
        const int it = tid + i * kThreads;
        const int h = it >= T::HP ? 1 : 0, pix = it - h * T::HP;
        const int hy = pix / T::HWID, hx = pix - hy * T::HWID;
        int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
        // rows / columns past the padded image belong to outputs that are never stored
        bool ok = it < 2 * T::HP && gy <= H && gx <= W;
        if (ok) ok = pad_coord(gy, H, a.pad_mode) & pad_coord(gx, W, a.pad_mode);
        off2[i] = ok ? gy * W + gx : -1;
        off1[i] = ok ? (a.up1 == 2 ? (gy >> 1) * a.W1 + (gx >> 1) : gy * a.W1 + gx) : -1;
        xdst[i] = it < 2 * T::HP ? x_lds_off(pix, h) : -1;
        xch[i] = 8 * h;
    }
    int wsrc[T::NWP];   // piece index of chunk 0 in the packed image (-1: a slab past Cout, staged as zeros)
#pragma unroll
    for (int i = 0; i < T::NWP; ++i) {
        const int q = tid + i * kThreads;
        const int mp = q / kChunkPieces, r = q - mp * kChunkPieces, m = mp / T::PL, pl = mp - m * T::PL;
        const int cot = cot0 + m;
        wsrc[i] = (q < T::WPIECES && cot * 32 < a.Cout) ? pl * a.plane_pieces + cot * a.nchunks * kChunkPieces + r : -1;
    }

    float xv[T::NIT][8];
    u32x4 wv[T::NWP];
    auto load_chunk = [&](int c) {
        const int ch0 = c * 16;
        const bool in1 = ch0 < a.C1;
        const float* src = in1 ? a.x1 + ((size_t)b * a.C1 + ch0) * plane1 : a.x2 + ((size_t)b * a.C2 + (ch0 - a.C1)) * plane2;
        const int plane = in1 ? plane1 : plane2;
#pragma unroll
        for (int i = 0; i < T::NIT; ++i) {
            const int off = in1 ? off1[i] : off2[i];
            const float* p = src + (size_t)xch[i] * plane + (off >= 0 ? off : 0);
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[i][j] = off >= 0 ? p[(size_t)j * plane] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < T::NWP; ++i)
            wv[i] = wsrc[i] >= 0 ? a.wp[wsrc[i] + c * kChunkPieces] : u32x4{0u, 0u, 0u, 0u};
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < T::NIT; ++i) {
            if (xdst[i] < 0) continue;
            bf16x8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                hi[j] = (__bf16)xv[i][j];
                if constexpr (TERMS == 3) lo[j] = (__bf16)(xv[i][j] - (float)hi[j]);
            }
            *reinterpret_cast<bf16x8*>(xs + xdst[i]) = hi;
            if constexpr (TERMS == 3) *reinterpret_cast<bf16x8*>(xs + T::X_PLANE_BYTES + xdst[i]) = lo;
        }
#pragma unroll
        for (int i = 0; i < T::NWP; ++i)
            if (tid + i * kThreads < T::WPIECES) *reinterpret_cast<u32x4*>(ws + (tid + i * kThreads) * 16) = wv[i];
    };

    const int hsel = lane >> 5, lp = lane & 31;
    int pbase[NR];
#pragma unroll
    for (int n = 0; n < NR; ++n) {
        const int p = (wave * NR + n) * 32 + lp;
        pbase[n] = (p / TW) * T::HWID + (p % TW);
    }
    f32x16 acc[MR][NR];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int n = 0; n < NR; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    if (c_begin < c_end) load_chunk(c_begin);
    for (int c = c_begin; c < c_end; ++c) {
        store_chunk();
        __syncthreads();
        if (c + 1 < c_end) load_chunk(c + 1);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            bf16x8 bh[NR], bl[NR], ah[MR], al[MR];
#pragma unroll
            for (int n = 0; n < NR; ++n) {
                const int off = x_lds_off(pbase[n] + (tap / 3) * T::HWID + (tap % 3), hsel);
                bh[n] = *reinterpret_cast<const bf16x8*>(xs + off);
                if constexpr (TERMS == 3) bl[n] = *reinterpret_cast<const bf16x8*>(xs + T::X_PLANE_BYTES + off);
            }
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                ah[m] = *reinterpret_cast<const bf16x8*>(ws + ((m * T::PL) * 9 + tap) * 1024 + lane * 16);
                if constexpr (TERMS == 3) al[m] = *reinterpret_cast<const bf16x8*>(ws + ((m * T::PL + 1) * 9 + tap) * 1024 + lane * 16);
            }
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int n = 0; n < NR; ++n) {
                    if constexpr (TERMS == 3) {
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[m], bh[n], acc[m][n], 0, 0, 0);
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[m], bl[n], acc[m][n], 0, 0, 0);
                    }
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[m], bh[n], acc[m][n], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    // epilogue: lane = pixel, register r = output channel (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the slab
    const size_t fr = (size_t)a.Cout * plane2;
    float* const yb = a.y + ((size_t)ks * a.B + b) * fr;
    const bool final_ = a.ksplit == 1;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        const int co0 = (cot0 + m) * 32;
        if (co0 >= a.Cout) continue;
#pragma unroll
        for (int n = 0; n < NR; ++n) {
            const int p = (wave * NR + n) * 32 + lp;
            const int oy = y0 + p / TW, ox = x0 + p % TW;
            if (oy >= H || ox >= W) continue;
            float* const dst = yb + (size_t)oy * W + ox;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * hsel;
                float v = acc[m][n][r];
                if (final_) v = epi_act(v + (a.bias ? a.bias[co] : 0.f), a.act, a.slope);
                dst[(size_t)co * plane2] = v;
            }
        }
    }
}

// second stage of a split reduction: slices summed in slice order (bit-repeatable), then bias + activation
__global__ __launch_bounds__(256) void conv_bf16_splitk_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                                      float* __restrict__ y, size_t n, size_t plane, int Cout,
                                                                      int ksplit, int act, float slope) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v = 0.f;
        for (int s = 0; s < ksplit; ++s) v += part[(size_t)s * n + i];
        const int co = (int)((i / plane) % Cout);
        y[i] = epi_act(v + (bias ? bias[co] : 0.f), act, slope);
    }
}

// [Cout,Cin,3,3] fp32 -> fragment image: piece (plane, slab, chunk, tap, lane) holds w[slab*32 + (lane & 31)][chunk*16 + 8 (lane >> 5) + j][tap],
// j = 0..7, as bf16(w) in plane 0 and bf16(w - bf16(w)) in plane 1
__global__ __launch_bounds__(256) void conv_bf16_pack_kernel(const float* __restrict__ w, bf16x8* __restrict__ wp, int Cout, int Cin, int planes) {
    const int nchunks = Cin / 16, per_plane = (Cout / 32) * nchunks * kChunkPieces;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < per_plane; q += gridDim.x * 256) {
        const int ln = q & 63, tap = (q >> 6) % 9, cc = (q / kChunkPieces) % nchunks, cot = q / (kChunkPieces * nchunks);
        const int co = cot * 32 + (ln & 31), ci0 = cc * 16 + 8 * (ln >> 5);
        bf16x8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = w[((size_t)co * Cin + ci0 + j) * 9 + tap];
            hi[j] = (__bf16)v;
            lo[j] = (__bf16)(v - (float)hi[j]);
        }
        wp[q] = hi;
        if (planes == 2) wp[per_plane + q] = lo;
    }
}

struct Bf16Cfg {
    const char* name;        // tile arguments TH,TW,MR,NR; the profiler appends TERMS
    const char* name_t[2];   // TERMS = 1, 3
    int TH, TW, MR, NR;
    int lds_bytes[2];
    void (*launch[2])(const Bf16KArgs&, dim3, hipStream_t);
};

template <int TH, int TW, int MR, int NR, int TERMS>
void launch_bf16(const Bf16KArgs& a, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((conv_bf16_kernel<TH, TW, MR, NR, TERMS>), grid, dim3(kThreads), 0, s, a);
}

#define WMD_BF16_CFG(TH, TW, MR, NR)                                                                                        \
    {"conv_bf16_kernel<" #TH "," #TW "," #MR "," #NR ">",                                                                   \
     {"conv_bf16_kernel<" #TH "," #TW "," #MR "," #NR ",1>", "conv_bf16_kernel<" #TH "," #TW "," #MR "," #NR ",3>"},          \
     TH, TW, MR, NR,                                                                                                        \
     {B16Tile<TH, TW, MR, NR, 1>::LDS_BYTES, B16Tile<TH, TW, MR, NR, 3>::LDS_BYTES},                                        \
     {launch_bf16<TH, TW, MR, NR, 1>, launch_bf16<TH, TW, MR, NR, 3>}}

const Bf16Cfg kBf16Cfgs[] = {
    WMD_BF16_CFG(8, 32, 2, 2),    // 64 channels x 256 pixels: the fine levels
    WMD_BF16_CFG(8, 32, 1, 2),    // 32 x 256
    WMD_BF16_CFG(4, 32, 2, 1),    // 64 x 128
    WMD_BF16_CFG(8, 16, 2, 1),    // 64 x 128, narrow: the coarse levels (20 and 40 pixel rows)
    WMD_BF16_CFG(8, 16, 1, 1),    // 32 x 128
};
constexpr int kNumBf16Cfgs = (int)(sizeof(kBf16Cfgs) / sizeof(kBf16Cfgs[0]));

struct Bf16Plan {
    const Bf16Cfg* cfg;
    int tiles_x, tiles_y, cob, nchunks, ksplit, cps;
    size_t workspace_floats;
};

// the operator's contract, then the family's own shape / feature rules of include/wmd.h (no tensor pointer is read: the
// queries answer from this); 0 or a negative status with the error text set
int bf16_rules(const wmd_conv_args* g, int terms, const char* who) {
    if (!g) return fail(WMD_ERR_BAD_ARG, "%s: null args", who);
    if (terms != 1 && terms != 3) return fail(WMD_ERR_BAD_ARG, "%s: terms=%d (1 or 3)", who, terms);
    const int st = conv_check_problem(g->B, g->H, g->W, g->C1, g->up1, g->C2, g->Cout, g->ksize, g->pad_mode, g->act, who);
    if (st) return st;
    if (g->ksize != 3) return fail(WMD_ERR_UNSUPPORTED, "%s: ksize=%d (3x3 only)", who, g->ksize);
    if (g->pad_mode == WMD_PAD_REPLICATE) return fail(WMD_ERR_UNSUPPORTED, "%s: replicate padding", who);
    if (g->gate) return fail(WMD_ERR_UNSUPPORTED, "%s: gate is not implemented by the bf16 kernels", who);
    if (g->in_mask || g->out_mask || g->out_tiles)
        return fail(WMD_ERR_UNSUPPORTED, "%s: in_mask / out_mask / out_tiles are not implemented by the bf16 kernels", who);
    if (g->C1 % 16 || g->C2 % 16 || g->Cout % 32)
        return fail(WMD_ERR_UNSUPPORTED, "%s: channels C1=%d C2=%d Cout=%d (C1, C2 multiples of 16, Cout of 32)", who, g->C1, g->C2, g->Cout);
    const double lim = 2147483647.0;
    const double hw = (double)g->H * g->W;
    if ((double)g->C1 * hw / (g->up1 * g->up1) * 4 > lim || (double)g->C2 * hw * 4 > lim || (double)g->Cout * hw * 4 > lim ||
        (double)g->Cout * (g->C1 + g->C2) * 9 * 4 > lim)
        return fail(WMD_ERR_UNSUPPORTED, "%s: a per-image tensor slice or the weight image exceeds 2 GiB", who);
    return WMD_OK;
}

// library's own choice: fewest machine rounds of (MR x NR MFMA tiles + a fixed staging share) per block, two blocks per CU
int bf16_plan(const wmd_conv_args* g, Bf16Plan* p, const char* who) {
    const int nchunks = (g->C1 + g->C2) / 16, ncot = g->Cout / 32;
    const int slots = 2 * kNumCU;
    int pick = -1;
    if (g->tune_cfg > 0) {
        if (g->tune_cfg > kNumBf16Cfgs) return fail(WMD_ERR_UNSUPPORTED, "%s: tune_cfg=%d (table has %d entries)", who, g->tune_cfg, kNumBf16Cfgs);
        pick = g->tune_cfg - 1;
    } else if (g->tune_cfg < 0) {
        return fail(WMD_ERR_UNSUPPORTED, "%s: tune_cfg=%d", who, g->tune_cfg);
    } else {
        double best = 0.0;
        for (int i = 0; i < kNumBf16Cfgs; ++i) {
            const Bf16Cfg& c = kBf16Cfgs[i];
            const double blocks = (double)g->B * ((g->W + c.TW - 1) / c.TW) * ((g->H + c.TH - 1) / c.TH) * ((ncot + c.MR - 1) / c.MR);
            const double rounds = blocks < slots ? 1.0 : blocks / slots;    // (a partly filled machine still takes one round)
            const double t = rounds * (c.MR * c.NR + 0.75);
            if (pick < 0 || t < best) pick = i, best = t;
        }
    }
    const Bf16Cfg& c = kBf16Cfgs[pick];
    p->cfg = &c;
    p->tiles_x = (g->W + c.TW - 1) / c.TW;
    p->tiles_y = (g->H + c.TH - 1) / c.TH;
    p->cob = (ncot + c.MR - 1) / c.MR;
    p->nchunks = nchunks;
    const size_t blocks = (size_t)g->B * p->tiles_x * p->tiles_y * p->cob;
    int want = 1;
    bool forced = false;
    if (g->tune_ksplit != 0) {
        want = std::min(std::abs(g->tune_ksplit), nchunks);
        forced = want > 1;
    } else if (blocks < (size_t)slots && nchunks >= 8) {   // coarse levels: fill the machine, at least four chunks per slice
        want = (int)std::min<size_t>(std::min((size_t)nchunks / 4, (slots + blocks - 1) / blocks), 16);
    }
    p->cps = (nchunks + want - 1) / want;
    p->ksplit = (nchunks + p->cps - 1) / p->cps;
    p->workspace_floats = p->ksplit > 1 ? (size_t)p->ksplit * g->B * g->Cout * g->H * g->W : 0;
    return forced ? 1 : 0;
}

}  // namespace
}  // namespace wmd

using namespace wmd;

extern "C" int wmd_conv_bf16_num_configs(void) { return kNumBf16Cfgs; }
extern "C" const char* wmd_conv_bf16_config_name(int i) { return (i >= 0 && i < kNumBf16Cfgs) ? kBf16Cfgs[i].name : nullptr; }

extern "C" size_t wmd_conv_bf16_packed_weight_bytes(int Cout, int Cin, int terms) {
    if ((terms != 1 && terms != 3) || Cout <= 0 || Cin <= 0 || Cout % 32 || Cin % 16) return 0;
    return (size_t)2 * 9 * Cout * Cin * (terms == 3 ? 2 : 1);
}

extern "C" int wmd_conv_bf16_pack_weights(const float* w, void* wp, int Cout, int Cin, int terms, void* stream) {
    if (!w || !wp) return fail(WMD_ERR_BAD_ARG, "wmd_conv_bf16_pack_weights: null pointer");
    if (terms != 1 && terms != 3) return fail(WMD_ERR_BAD_ARG, "wmd_conv_bf16_pack_weights: terms=%d (1 or 3)", terms);
    if (!wmd_conv_bf16_packed_weight_bytes(Cout, Cin, terms))
        return fail(WMD_ERR_UNSUPPORTED, "wmd_conv_bf16_pack_weights: Cout=%d Cin=%d (multiples of 32 and 16)", Cout, Cin);
    const int per_plane = (Cout / 32) * (Cin / 16) * kChunkPieces;
    ProfScope prof("conv_bf16_pack_kernel", 0.0, 4.0 * 9 * Cout * Cin + (double)wmd_conv_bf16_packed_weight_bytes(Cout, Cin, terms), (hipStream_t)stream);
    hipLaunchKernelGGL(conv_bf16_pack_kernel, dim3(std::min((per_plane + 255) / 256, 2048)), dim3(256), 0, (hipStream_t)stream, w,
                       (bf16x8*)wp, Cout, Cin, terms == 3 ? 2 : 1);
    return check_launch("conv_bf16_pack_kernel");
}

extern "C" int wmd_conv_bf16_supported(const wmd_conv_args* g, int terms) {
    if (bf16_rules(g, terms, "wmd_conv_bf16_supported")) return 0;
    Bf16Plan plan;
    return bf16_plan(g, &plan, "wmd_conv_bf16_supported") >= 0 ? 1 : 0;
}

extern "C" size_t wmd_conv_bf16_workspace_floats(const wmd_conv_args* g, int terms) {
    if (bf16_rules(g, terms, "wmd_conv_bf16_workspace_floats")) return 0;
    Bf16Plan plan;
    if (bf16_plan(g, &plan, "wmd_conv_bf16_workspace_floats") < 0) return 0;
    return plan.workspace_floats;
}

extern "C" int wmd_conv_bf16_fwd(const wmd_conv_args* g, int terms, void* stream) {
    const char* who = "wmd_conv_bf16_fwd";
    int st = bf16_rules(g, terms, who);
    if (!st) st = conv_check_tensors(g, who);
    if (st) return st;
    Bf16Plan plan;
    const int forced = bf16_plan(g, &plan, who);
    if (forced < 0) return forced;
    if (plan.ksplit > 1 && (!g->workspace || g->workspace_floats < plan.workspace_floats)) {
        if (forced)
            return fail(WMD_ERR_WORKSPACE, "%s: a %d-way split needs a workspace of %zu floats (got %zu)", who, plan.ksplit,
                        plan.workspace_floats, g->workspace ? g->workspace_floats : (size_t)0);
        plan.ksplit = 1;   // the library's own split is an option, not a need
        plan.cps = plan.nchunks;
        plan.workspace_floats = 0;
    }
    const Bf16Cfg& c = *plan.cfg;
    const int ti = terms == 3 ? 1 : 0;
    Bf16KArgs a;
    memset(&a, 0, sizeof(a));
    a.x1 = g->x1;
    a.x2 = g->C2 > 0 ? g->x2 : nullptr;
    a.wp = (const u32x4*)g->wp;
    a.bias = g->bias;
    a.y = plan.ksplit > 1 ? g->workspace : g->y;
    a.B = g->B;
    a.H = g->H;
    a.W = g->W;
    a.H1 = g->H / g->up1;
    a.W1 = g->W / g->up1;
    a.C1 = g->C1;
    a.C2 = g->C2;
    a.Cout = g->Cout;
    a.up1 = g->up1;
    a.pad_mode = g->pad_mode;
    a.act = g->act;
    a.slope = g->slope;
    a.tiles_x = plan.tiles_x;
    a.tiles_y = plan.tiles_y;
    a.cob = plan.cob;
    a.nchunks = plan.nchunks;
    a.ksplit = plan.ksplit;
    a.cps = plan.cps;
    a.plane_pieces = (g->Cout / 32) * plan.nchunks * kChunkPieces;
    const int Cin = g->C1 + g->C2;
    const double pix = (double)g->B * g->H * g->W;
    const dim3 grid((unsigned)((size_t)g->B * plan.tiles_x * plan.tiles_y * plan.cob), (unsigned)plan.ksplit);
    {
        const double flops = 2.0 * Cin * 9 * g->Cout * pix;
        ProfScope prof(c.name_t[ti], flops,
                       4.0 * (pix * g->C1 / (g->up1 * g->up1) + pix * g->C2 + pix * g->Cout) + (double)wmd_conv_bf16_packed_weight_bytes(g->Cout, Cin, terms),
                       (hipStream_t)stream);
        prof.mfma(terms * flops);
        c.launch[ti](a, grid, (hipStream_t)stream);
    }
    st = check_launch("conv_bf16_kernel");
    if (st) return st;
    if (plan.ksplit > 1) {
        const size_t n = (size_t)g->B * g->Cout * g->H * g->W;
        const int blocks = (int)std::min<size_t>((n + 255) / 256, 2048);
        ProfScope prof("conv_bf16_splitk_reduce_kernel", (double)n * plan.ksplit, 4.0 * n * (plan.ksplit + 1), (hipStream_t)stream);
        hipLaunchKernelGGL(conv_bf16_splitk_reduce_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g->workspace, g->bias, g->y, n,
                           (size_t)g->H * g->W, g->Cout, plan.ksplit, g->act, g->slope);
        st = check_launch("conv_bf16_splitk_reduce_kernel");
    }
    return st;
}
