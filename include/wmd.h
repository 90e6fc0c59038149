/*
 * wmd.h — C ABI of libwmd_hip.so: the MI355X (gfx950) implementation of the
 * wavelet-monodepth decoder + Haar IDWT/DWT hot path.
 *
 * The reference (nianticlabs/wavelet-monodepth) has no FFI layer: its boundary
 * for this path is the Python nn.Module surface.  Every entry
 * point below therefore names the reference *operator* it replaces (file:line
 * under /root/reference) — these are what a maintainer binds with ctypes from
 * the decoder modules.
 *
 * Conventions
 *   - all tensors fp32, NCHW, contiguous, device memory owned by the caller
 *   - every call is asynchronous, ordered on `stream` (a hipStream_t passed as void*)
 *   - return value: 0 (WMD_OK) or a negative wmd_status; nothing throws
 *   - the library keeps no state besides a thread-local last-error string
 */
#ifndef WMD_H
#define WMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WMD_VERSION 100 /* 0.1.0 */

typedef enum {
    WMD_OK = 0,
    WMD_ERR_BAD_ARG = -1,     /* null pointer, negative size, unknown enum */
    WMD_ERR_BAD_SHAPE = -2,   /* shape the reference op itself would reject  */
    WMD_ERR_UNSUPPORTED = -3, /* valid but not implemented                   */
    WMD_ERR_HIP = -4,         /* a HIP runtime call or launch failed         */
    WMD_ERR_WORKSPACE = -5,   /* caller-provided workspace too small         */
    WMD_ERR_COMM = -6         /* RCCL failure                                */
} wmd_status;

/* padding applied before a 3x3 convolution
 *   ZERO      nn.ZeroPad2d(1)        KITTI/layers.py:155, NYUv2/networks/layers.py:22
 *   REFLECT   nn.ReflectionPad2d(1)  KITTI/layers.py:153, NYUv2/networks/layers.py:18
 *   REPLICATE nn.ReplicationPad2d(1) NYUv2/networks/layers.py:20                     */
typedef enum { WMD_PAD_ZERO = 0, WMD_PAD_REFLECT = 1, WMD_PAD_REPLICATE = 2 } wmd_pad;

/* activation fused after bias
 *   ELU (alpha=1)  KITTI/layers.py:131      LEAKY(slope) depth_decoder.py:105, NYUv2 layers.py:61
 *   SIGMOID        depth_decoder.py:133     */
typedef enum { WMD_ACT_NONE = 0, WMD_ACT_ELU = 1, WMD_ACT_LEAKY = 2, WMD_ACT_SIGMOID = 3 } wmd_act;

int wmd_version(void);
const char* wmd_last_error(void);
const char* wmd_status_string(int status);

/* Opt-in kernel timing (the only process-global state in the library; not thread-safe).
 * Between begin and end every kernel launch of this library is bracketed by a hipEvent pair on
 * its launch stream.  wmd_profile_end synchronises and writes a JSON array
 *   [{"kernel": name, "calls": n, "ms": total, "flops": algorithmic FLOPs, "bytes": algorithmic bytes,
 *     "mfma_flops": FLOPs the matrix pipe executes (Winograd kernels: fewer than algorithmic)}, ...]
 * into buf (truncated to cap); returns the number of bytes needed, or a negative wmd_status.    */
int wmd_profile_begin(void);
long wmd_profile_end(char* buf, size_t cap);

/* ------------------------------------------------------------------ *
 * Haar wavelets  (third-party pytorch_wavelets; call sites
 * KITTI/networks/decoders/depth_decoder.py:85,164,372,416,
 * NYUv2/networks/decoders/densedepth_decoder.py:99,129,137,145, NYUv2/train.py:258,289;
 * closed form restated by the authors at depth_decoder.py:225-239)
 * ------------------------------------------------------------------ */

/* IDWT(wave="haar", mode="zero"), one level.
 *   yl [N,h,w], yh [N,3,h,w] (LH,HL,HH)  ->  out [N,2h,2w]
 *   if disp != NULL also writes disp = out*disp_scale, clamped to [0,1] when clamp01 != 0
 *   (depth_decoder.py:166 `clamp(yl / 2**(i-1), 0, 1)`; NYUv2 decoder: scale only).
 *   N = batch*channels (channels is 1 everywhere in the reference).
 *   Alignment: with an even w the kernel loads float2 and stores float4 through these pointers, so yl and yh must be
 *   8-byte and out and disp 16-byte aligned (WMD_ERR_BAD_ARG otherwise, nothing launched); an odd w runs a scalar
 *   kernel and needs only the 4 bytes of a float.  Tensors are dense: no strides.       */
int wmd_idwt_haar_fwd(const float* yl, const float* yh, float* out, float* disp,
                      int N, int h, int w, float disp_scale, int clamp01, void* stream);

/* Adjoint of the above.  d_out [N,2h,2w] (may be NULL = zero), d_disp [N,2h,2w] (may be NULL);
 * `out` is the forward result (needed for the clamp mask when d_disp != NULL && clamp01).
 * Writes d_yl [N,h,w] and d_yh [N,3,h,w].
 * Alignment: d_out, d_disp and out are read as float2 and must be 8-byte aligned whatever w is (WMD_ERR_BAD_ARG
 * otherwise, nothing launched); d_yl and d_yh are stored float by float.                */
int wmd_idwt_haar_bwd(const float* d_out, const float* d_disp, const float* out,
                      float* d_yl, float* d_yh, int N, int h, int w,
                      float disp_scale, int clamp01, void* stream);

/* DWT(J=1, wave="haar", mode="reflect"/"zero") on even H,W (the only case the reference hits,
 * NYUv2/train.py:258 on 240x320 depth): x [N,2h,2w] -> yl [N,h,w], yh [N,3,h,w].
 * Call J times for a J-level transform (yh list is fine -> coarse).
 * Alignment: x is read as float2 and must be 8-byte aligned (WMD_ERR_BAD_ARG otherwise); yl, yh: 4 bytes.   */
int wmd_dwt_haar_fwd(const float* x, float* yl, float* yh, int N, int h, int w, void* stream);
/* The same analysis step for ANY input size H x W (mode="reflect" of pytorch_wavelets' DWTForward, NYUv2/train.py:258):
 * an odd axis is extended by one reflected sample on the right / bottom (x[N] = x[N-2]) before the stride-2 filter
 * pair, so yl [N,ceil(H/2),ceil(W/2)], yh [N,3,ceil(H/2),ceil(W/2)].  An odd axis needs >= 2 samples.  Scalar loads and
 * stores: every pointer needs only a float's 4-byte alignment.                                                        */
int wmd_dwt_haar_reflect_fwd(const float* x, float* yl, float* yh, int N, int H, int W, void* stream);

/* ------------------------------------------------------------------ *
 * Dense convolutions of the decoders (implicit GEMM on fp32 MFMA)
 * ------------------------------------------------------------------ */

/* Number of floats of the MFMA-fragment-ordered weight image for a [Cout,Cin,k,k] filter. */
size_t wmd_conv_packed_weight_floats(int Cout, int Cin, int ksize);

/* Re-order nn.Conv2d weights [Cout,Cin,k,k] (k = 1 or 3) into the fragment image `wp`
 * the conv kernels read (16 out-channels x 4 in-channels per 256-byte wave load).       */
int wmd_conv_pack_weights(const float* w, float* wp, int Cout, int Cin, int ksize, void* stream);

/* Same re-ordering for the data-gradient pass: transposes in/out channels and flips taps. */
int wmd_conv_pack_weights_dgrad(const float* w, float* wp, int Cout, int Cin, int ksize, void* stream);

typedef struct {
    int B, H, W;        /* output size; also the logical input size (stride 1, "same")  */
    int C1;             /* channels of x1                                              */
    int up1;            /* 1: x1 is [B,C1,H,W]; 2: x1 is [B,C1,H/2,W/2], nearest x2    */
    int C2;             /* channels of the skip tensor x2 [B,C2,H,W]; 0 if none        */
    int Cout;
    int ksize;          /* 1 or 3                                                      */
    int pad_mode;       /* wmd_pad (ignored for ksize 1)                               */
    int act;            /* wmd_act                                                     */
    float slope;        /* LeakyReLU negative slope                                    */
    const float* x1;
    const float* x2;    /* may be NULL when C2 == 0                                    */
    const float* wp;    /* packed weights (wmd_conv_pack_weights) for Cin = C1 + C2    */
    const float* bias;  /* [Cout] or NULL                                              */
    float* y;           /* [B,Cout,H,W]                                                */
    float* workspace;   /* split-K partial sums; may be NULL -> never split            */
    size_t workspace_floats;
    int tune_cfg;       /* 0: built-in cost model; k>0: force tile configuration k-1     */
    int tune_ksplit;    /* 0: cost model; k>0: force k-way split of the Cin reduction,
                           finished inside the convolution where the kernel can (the
                           32x32x2 Winograd kernels: the last K-slice block of a tile sums
                           the slices -- same order, same bits as the second-stage kernel);
                           k<0: |k| slices summed by the second-stage kernel (only for
                           kernels that have both forms; WMD_ERR_UNSUPPORTED otherwise)     */
    const float* wp_wino; /* optional (3x3 only): wmd_conv_pack_weights_wino image; enables the Winograd F(2x2,3x3)
                             configurations ("conv_wino_kernel<...>": 2.25x fewer MFMAs, ~1e-6 relative rounding) */
    const float* gate;  /* optional [B,Cout,H,W]: y = act(conv + bias) * act_gate'(gate), the derivative written in terms of
                           an activation OUTPUT (ELU: g > 0 ? 1 : g + 1; LeakyReLU: g > 0 ? 1 : slope).  Lets a consumer's
                           data gradient hand the producer dz = dy * f'(y) directly (no separate wmd_act_bwd pass).
                           Direct kernels only (the Winograd configurations are skipped when it is set).             */
    int gate_act;       /* wmd_act of the gate                                          */
    float gate_slope;
    /* Block-sparse execution (3x3; the threshold-gated sparse decoders on the dense MFMA kernels when several frames are
     * decoded together): with out_mask [B,H,W] only the pixel tiles that contain an active output pixel are computed (every
     * block tests its own tile's mask bytes and returns when there is none), outputs outside the mask are written as 0 and
     * tiles without active pixels are NOT touched (y must be zero-initialised -- or every consumer of y must select on the
     * mask rather than multiply by it, which is how the sparse decoders use their never-refilled activation pool: the next
     * layer's in_mask / the head's yh_mask gate every read, tests/test_gpu_configs.py poisons the pool with NaN); with in_mask
     * [B,H,W] a padded input
     * position outside the mask reads 0 for x1 and x2 alike -- the mask test after the coordinate padding of
     * sparse_conv3x3 (KITTI/layers.py:439-453).  Split-K stays available (the reduce pass writes 0 outside out_mask and
     * never reads the slots of a skipped tile); implemented by the Winograd kernels (needs wp_wino).
     * in_mask_2x2 != 0 is the caller's promise that in_mask is constant on aligned 2x2 pixel blocks (it is the nearest
     * upsampling of a half-resolution mask, as the decoders' upsample mask is: MaxPool5(upsample(m)) = upsample(MaxPool3(m)));
     * with up1 = 2 it lets the upsampled operand keep the structured low-resolution path of conv_wino32_kernel (the mask
     * of source pixel (y, x) is read at (2y, 2x)).  Without the promise a masked upsampled layer runs the generic gather.  */
    const uint8_t* in_mask;
    const uint8_t* out_mask;
    int in_mask_2x2;
    /* Work-list form of the block-sparse execution (round 4; wmd_mask_level_lists builds the list).  out_tiles holds the
     * indices ((b * tiles_y + ty) * tiles_x + tx, tiles of out_tile_h x out_tile_w pixels) of the pixel tiles that contain
     * an active pixel of out_mask, per frame: out_tiles [B][tiles_y * tiles_x], out_tile_count [B] (frame f's tiles are the
     * first out_tile_count[f] entries of its segment, in any order).  Only listed tiles are
     * dispatched to a matrix-pipe workgroup -- an unlisted tile costs nothing and, as before, is not written -- and the
     * split of the input-channel reduction is chosen ON THE DEVICE from the count (few active tiles: every tile's K loop is
     * spread over many workgroups, whose partial sums meet in a list-driven second pass; many: no split, no second pass
     * work), so that the time follows the active work.  Needs out_mask, a 3x3 layer, wp_wino, a `pure` channel layout
     * (C1, C2 multiples of 8; an upsampled x1 needs in_mask_2x2) and a tile shape the library has a list kernel for
     * (wmd_conv_list_tile_supported); workspace: wmd_conv_fwd_workspace_floats.  Values: identical to the mask form.     */
    const int32_t* out_tiles;
    const int32_t* out_tile_count;
    int out_tile_h, out_tile_w;
} wmd_conv_args;

/* The contract of this problem.  Every entry point that takes it (wmd_conv_fwd, the bf16 and F(4x4,3x3) families, wmd_conv_dgrad,
 * wmd_conv_wgrad, the depthwise 3x3 with Cout = 1 and ksize = 3, wmd_sparse_conv with max(B, 1) frames) applies the same rules
 * before any rule of its own and before any HIP call, and reports the first one violated, in this order:
 *   B, H, W, C1, Cout >= 1 and C2 >= 0 (WMD_ERR_BAD_SHAPE); ksize 1 or 3 (WMD_ERR_UNSUPPORTED); up1 1 or 2 (WMD_ERR_BAD_ARG);
 *   even H and W when up1 = 2 (WMD_ERR_BAD_SHAPE); pad_mode a wmd_pad (WMD_ERR_BAD_ARG); act a wmd_act, where the entry has one
 *   (WMD_ERR_BAD_ARG); H, W >= 2 for a 3x3 filter with REFLECT padding (WMD_ERR_BAD_SHAPE).
 * None of them reads a pointer.  An entry that launches then needs x1, wp and y, and x2 when C2 > 0 (WMD_ERR_BAD_ARG); the
 * shape queries (*_supported, *_workspace_floats, wmd_conv_fwd_plan) ignore these four pointers.                                */

/* != 0 when wmd_conv_fwd has a work-list kernel for pixel tiles of tile_h x tile_w */
int wmd_conv_list_tile_supported(int tile_h, int tile_w);

/* Fused  upsample(x1) ++ x2  ->  pad  ->  conv kxk  ->  + bias  ->  activation.
 * Replaces ConvBlock/Conv3x3/Conv1x1 (KITTI/layers.py:120-173), `upsample` (:233-236),
 * the skip `torch.cat` (depth_decoder.py:146-149), NYUv2 Conv3x3/UpSampleBlock
 * (NYUv2/networks/layers.py:11-32,57-67).                                              */
int wmd_conv_fwd(const wmd_conv_args* args, void* stream);

/* Suggested workspace size (floats) for wmd_conv_fwd on this problem. */
size_t wmd_conv_fwd_workspace_floats(const wmd_conv_args* args);

/* What wmd_conv_fwd would run on this problem, given a workspace of any size (host code: no launch, no pointer is
 * dereferenced): the table index of the chosen configuration (wmd_conv_config_name), or -1 when no entry takes the
 * problem; *ksplit (may be NULL) receives the number of K slices.  tune_cfg / tune_ksplit are honoured as in wmd_conv_fwd;
 * with both 0 this is the cost model's own choice (stream captures on a tuner miss, WMD_AUTOTUNE=0).                  */
int wmd_conv_fwd_plan(const wmd_conv_args* args, int* ksplit);

/* Winograd-domain weight image of a 3x3 filter: U = G g G^T per (out, in) channel pair, in the fragment order of
 * wmd_conv_pack_weights with 16 transformed positions in place of the 9 taps.  dgrad != 0: the transposed / flipped
 * filter of the data-gradient pass.                                                                              */
size_t wmd_conv_packed_weight_floats_wino(int Cout, int Cin);
int wmd_conv_pack_weights_wino(const float* w, float* wp, int Cout, int Cin, int dgrad, void* stream);

/* Every weight image of a set of filters in ONE launch (training repacks all of them after each optimizer step).  Each
 * non-NULL output receives exactly what the single-filter entry point writes: fwd = wmd_conv_pack_weights, dgrad =
 * wmd_conv_pack_weights_dgrad, wino_fwd / wino_dgrad = wmd_conv_pack_weights_wino(dgrad = 0 / 1) (3x3 filters only).
 * Outputs may alias slices of one buffer (sizes: wmd_conv_packed_weight_floats[_wino]).                              */
typedef struct {
    const float* w;      /* [Cout,Cin,ksize,ksize]                                       */
    int Cout, Cin, ksize;
    float* fwd;
    float* dgrad;
    float* wino_fwd;
    float* wino_dgrad;
} wmd_pack_item;
int wmd_conv_pack_many(const wmd_pack_item* items, int n, void* stream);

/* Tile-configuration table (for callers that autotune: wavelet_monodepth_amd/tuner.py).
 * wmd_conv_config_name returns e.g. "conv_fwd_kernel<8,32,2,4,1,4,8,9>" (the kernel's template
 * arguments TH,TW,MR,NR,WM,WN,CK,TAPS) or NULL when i is out of range.                        */
int wmd_conv_num_configs(void);
const char* wmd_conv_config_name(int i);

/* ------------------------------------------------------------------ *
 * Opt-in reduced precision for the 3x3 trunk convolutions: bf16 MFMA (v_mfma_f32_32x32x16_bf16), fp32 accumulate.
 * Tensors stay fp32 NCHW exactly as for wmd_conv_fwd; the operands are rounded on load.  With q(v) = fp32 -> bf16
 * round-to-nearest-even:
 *   terms = 1   y = act( sum_k q(x_k) q(w_k) + bias )                                   ~3e-3 of the tensor scale end to end
 *   terms = 3   y = act( sum_k [ q(x_k) q(w_k) + q(x_k) q(w_k - q(w_k)) + q(x_k - q(x_k)) q(w_k) ] + bias )      ~1e-5
 * (products of two bf16 values are exact in fp32; the sum is fp32 in an unspecified but fixed order: a launch is
 * bit-repeatable, there are no float atomics).  Same fusion as wmd_conv_fwd: nearest x2 upsample of x1, concat with x2, border
 * addressing, bias, activation.  wmd_conv_args is reused unchanged: wp = the image of wmd_conv_bf16_pack_weights, wp_wino is
 * ignored, tune_cfg = k > 0 forces entry k-1 of the table below (every entry runs every supported problem), tune_ksplit = k
 * (either sign) forces min(|k|, Cin/16) slices of the Cin reduction, summed in slice order by a second-stage kernel.
 * Supported, beyond the contract at wmd_conv_args (everything else WMD_ERR_UNSUPPORTED before any launch; wmd_conv_bf16_supported
 * and wmd_conv_bf16_workspace_floats answer for the problem without a HIP call and without reading x1, x2, wp or y):
 *   ksize = 3; pad ZERO or REFLECT; C1 % 16 == 0, C2 % 16 == 0, Cout % 32 == 0; gate, in_mask, out_mask, out_tiles NULL;
 *   tune_cfg in 0 .. wmd_conv_bf16_num_configs().
 * Packed weight image: bf16 in MFMA fragment order, plane q(w), then for terms = 3 plane q(w - q(w)):
 *   wmd_conv_bf16_packed_weight_bytes = 2 * 9 * Cout * Cin * (terms == 3 ? 2 : 1)      (0 unless Cout % 32 == 0, Cin % 16 == 0
 *   and terms is 1 or 3).
 * Workspace: a split needs slices * B*Cout*H*W floats.  wmd_conv_bf16_workspace_floats is what the library's choice (or the
 * forced split) wants; the library's own split is skipped when the workspace is NULL or smaller, a forced one is refused
 * (WMD_ERR_WORKSPACE).
 * wmd_conv_bf16_config_name: "conv_bf16_kernel<TH,TW,MR,NR>" (pixel tile TH x TW, MR x NR 32x32 MFMA tiles per wave); the
 * profiler reports launches as "conv_bf16_kernel<TH,TW,MR,NR,TERMS>" with mfma_flops = TERMS x flops.
 * ------------------------------------------------------------------ */
size_t wmd_conv_bf16_packed_weight_bytes(int Cout, int Cin, int terms);
int wmd_conv_bf16_pack_weights(const float* w, void* wp, int Cout, int Cin, int terms, void* stream);
int wmd_conv_bf16_supported(const wmd_conv_args* args, int terms);
size_t wmd_conv_bf16_workspace_floats(const wmd_conv_args* args, int terms);
int wmd_conv_bf16_fwd(const wmd_conv_args* args, int terms, void* stream);
int wmd_conv_bf16_num_configs(void);
const char* wmd_conv_bf16_config_name(int i);

/* ------------------------------------------------------------------ *
 * Winograd F(4x4,3x3) in three passes, for 3x3 layers with few pixels and many channels (the coarse up+skip layers of the
 * trunk): input transform V = B^T d B, 36 batched GEMMs M_p = U_p^T V_p on v_mfma_f32_32x32x2_f32, output transform
 * y = act(A^T M A + bias) -- "wino44_input_kernel", "wino44_gemm_kernel", "wino44_output_kernel" in the profiler.  36 matrix-
 * pipe positions per 16 outputs (the fused F(2x2,3x3) kernels execute 64); V and M live in the caller's workspace.  Same
 * operator and the same wmd_conv_args as wmd_conv_fwd: nearest x2 upsample of x1 (read at its own resolution: 25 of the 36
 * positions carry its channels), concat with x2, border addressing, bias, activation.  Points 0, +-1, +-2, inf: the rounding
 * error is ~2e-5 of the tensor's scale at 512 input channels (the fused F(2x2,3x3) kernels: 4e-7), which is why wmd_conv_fwd never chooses these
 * kernels by itself: a caller opts in per layer (ops.conv3x3_wino44_nograd, inference only).
 * Supported, beyond the contract at wmd_conv_args (everything else WMD_ERR_UNSUPPORTED before any launch; wmd_conv_wino44_supported
 * answers without a HIP call):
 *   ksize = 3; any C1, C2, Cout up to 65536; gate, in_mask, out_mask, out_tiles
 *   NULL; tune_cfg = tune_ksplit = 0 (one configuration; the reduction is never split: x1's channels, then x2's, in one
 *   workgroup -- a launch repeats bit for bit); every tensor and image below 2 GiB.
 * wp = the image of wmd_conv_pack_weights_wino44 for the same (Cout, C1, C2, up1): U = G g G^T computed in double and
 *   rounded once, [36][(C1p + C2p) / 4][Coutp][4] floats (channel counts rounded up to 32 each, Cout to 32); for up1 = 2 the rows of
 *   x1's channels are 0 at the 11 positions the upsampled operand does not reach (a replicated line transforms to 0 there).
 * Workspace: wmd_conv_wino44_workspace_floats(args) floats = V [36][(C1p + C2p) / 4][NTp][4] + M [36][Coutp][NTp] (NTp = the number of
 *   4x4 output tiles B ceil(H/4) ceil(W/4), rounded up to 32); smaller or NULL: WMD_ERR_WORKSPACE.  No host synchronisation:
 *   the three launches can be captured.
 * ------------------------------------------------------------------ */
size_t wmd_conv_packed_weight_floats_wino44(int Cout, int C1, int C2);
int wmd_conv_pack_weights_wino44(const float* w, float* wp, int Cout, int C1, int C2, int up1, void* stream);
int wmd_conv_wino44_supported(const wmd_conv_args* args);
size_t wmd_conv_wino44_workspace_floats(const wmd_conv_args* args);
int wmd_conv_wino44_fwd(const wmd_conv_args* args, void* stream);

/* dz = dy * act'(y)  (y = the activation OUTPUT saved by the forward). In place allowed.  Scalar loads and stores: 4-byte
 * alignment suffices.                                                                     */
int wmd_act_bwd(const float* dy, const float* y, float* dz, size_t n, int act, float slope, void* stream);

typedef struct {
    int B, H, W;        /* size of dz / of the logical (upsampled, concatenated) input   */
    int C1, up1, C2, Cout, ksize, pad_mode;
    const float* dz;    /* [B,Cout,H,W] gradient w.r.t. the pre-activation              */
    const float* wp_dgrad; /* wmd_conv_pack_weights_dgrad image                         */
    float* dx1;         /* [B,C1,H/up1,W/up1] or NULL                                   */
    float* dx2;         /* [B,C2,H,W] or NULL                                           */
    float* workspace;   /* needs wmd_conv_dgrad_workspace_floats                        */
    size_t workspace_floats;
    int tune_cfg;       /* as in wmd_conv_args: 0 = cost model, k > 0 forces configuration k-1 */
    int tune_ksplit;
    const float* wp_dgrad_wino; /* optional (3x3): wmd_conv_pack_weights_wino(..., dgrad = 1) image, enables Winograd */
    const float* x1_fwd; /* optional: the forward's x1 [B,C1,H/up1,W/up1], itself the OUTPUT of an activation x1_act: dx1 is
                            then multiplied by x1_act'(x1), i.e. it is already the producer's pre-activation gradient     */
    int x1_act;          /* wmd_act (WMD_ACT_NONE: no gating)                            */
    float x1_slope;
} wmd_conv_dgrad_args;

size_t wmd_conv_dgrad_workspace_floats(const wmd_conv_dgrad_args* args);
/* Data gradient: adjoint of pad + concat + nearest-upsample folded behind a full correlation. */
int wmd_conv_dgrad(const wmd_conv_dgrad_args* args, void* stream);

typedef struct {
    int B, H, W;
    int C1, up1, C2, Cout, ksize, pad_mode;
    const float* x1;
    const float* x2;
    const float* dz;    /* [B,Cout,H,W]                                                 */
    float* dw;          /* [Cout,C1+C2,k,k]  (overwritten)                              */
    float* dbias;       /* [Cout] or NULL    (overwritten)                              */
    float* workspace;
    size_t workspace_floats;
    int tune_cfg;       /* 0 = library model; k > 0 forces entry k-1 of the Winograd F(2x2,3x3) weight-gradient table
                           (wmd_conv_wgrad_num_configs / _config_name); -1 = direct kernel, library's tile.  k > num_configs,
                           k < -1, or k > 0 with ksize != 3 is refused (WMD_ERR_UNSUPPORTED; workspace_floats returns 0)   */
    int tune_nsplit;    /* 0 = library model; > 0 forces the number of pixel-tile slices (= partial sums)          */
} wmd_conv_wgrad_args;

/* the Winograd weight-gradient tile table (for autotuners; names are stable across versions) */
int wmd_conv_wgrad_num_configs(void);
const char* wmd_conv_wgrad_config_name(int index);

size_t wmd_conv_wgrad_workspace_floats(const wmd_conv_wgrad_args* args);
/* Weight + bias gradient (deterministic two-stage split over the B*H*W reduction). */
int wmd_conv_wgrad(const wmd_conv_wgrad_args* args, void* stream);

/* Depthwise 3x3 + ReLU over the same virtual input (upsample(x1) ++ x2, padded): the first half of the NYUv2 decoders'
 * optional `is_depthwise` Conv3x3 (NYUv2/networks/layers.py:23-25,70-79); its bias-free 1x1 second half is an
 * ordinary wmd_conv_fwd.  w [C1+C2,1,3,3]; y, dy [B,C1+C2,H,W].  Backward: dx1 / dx2 / dw may each be NULL.          */
typedef struct {
    int B, H, W;
    int C1, up1, C2, pad_mode;
    const float* x1;
    const float* x2;
    const float* w;
} wmd_dwconv_args;
int wmd_dwconv3x3_fwd(const wmd_dwconv_args* args, float* y, void* stream);
size_t wmd_dwconv3x3_bwd_workspace_floats(const wmd_dwconv_args* args);
int wmd_dwconv3x3_bwd(const wmd_dwconv_args* args, const float* y, const float* dy, float* dx1, float* dx2, float* dw,
                      float* workspace, size_t workspace_floats, void* stream);

/* ------------------------------------------------------------------ *
 * Wavelet heads: 3x3 convolutions with 1..3 output channels (HBM-bound)
 * ------------------------------------------------------------------ */
typedef struct {
    int B, H, W, C;     /* input [B,C,H,W]                                              */
    int Cout;           /* 1..4                                                         */
    int pad_mode;
    int mode;           /* 0: y = scale*conv_p(xp)                     (NYUv2 wave*, :122-141)
                           1: y = scale*sigmoid(conv_p(xp))            (LL head, depth_decoder.py:133)
                           2: y = scale*(sigmoid(conv_p(xp)) - sigmoid(conv_n(xn)))  (:134-135) */
    float scale;
    const float* xp; const float* wgt_p; const float* bias_p;   /* wgt [Cout,C,3,3]     */
    const float* xn; const float* wgt_n; const float* bias_n;   /* mode 2 only          */
    float* y;           /* [B,Cout,H,W]                                                 */
    float* sig_p;       /* optional [B,Cout,H,W]: sigmoid outputs saved for backward    */
    float* sig_n;
    size_t xp_bstride;  /* floats between consecutive batch items of xp / xn; 0 = C*H*W (lets xp, xn be  */
    size_t xn_bstride;  /* channel slices of one stacked [B,Ctot,H,W] tensor)                             */
    float* workspace;   /* optional (wmd_head3x3_workspace_floats): lets coarse levels split the channel  */
    size_t workspace_floats; /* loop over several workgroups (two-stage, deterministic)                   */
} wmd_head_args;

/* Replaces Conv3x3(C,3|1) + Sigmoid + the 2^(s-1)(sigma+ - sigma-) combine of
 * DepthWaveProgressiveDecoder.get_coefficients (depth_decoder.py:126-136) and the
 * NYUv2 wave1_ll/wave{1,2,3} convolutions (densedepth_decoder.py:106-115).             */
int wmd_head3x3_fwd(const wmd_head_args* args, void* stream);
size_t wmd_head3x3_workspace_floats(const wmd_head_args* args);

/* Fused inference form of a level's two high-frequency heads (depth_decoder.py:108-136):
 *   mid_s = LeakyReLU(W1_s x + b1_s)            s in {+,-}, both C -> C     (MFMA GEMM, result stays on chip: for C = 64,
 *                                                                            128, 256 in the accumulator registers, which are
 *                                                                            the next product's operand -- head_chain_kernel)
 *   t[s*27 + co*9 + tap] = sum_c W3_s[co,c,tap] * mid_s[c]                  (second MFMA GEMM of the same wave)
 * i.e. the 3x3 convolution regrouped as 27 tap-partial 1x1 outputs; wmd_head_shiftsum_fwd then gathers the
 * nine shifted taps, adds the bias, applies sigmoid / 2^(s-1)(sig+ - sig-) and (optionally) the Haar IDWT.
 * wp1: wmd_conv_pack_weights image of the stacked [2C, C, 1, 1] filter (+ rows first); bias1 [2C];
 * wp2: two wmd_conv_pack_weights images of [27, C, 1, 1] (W3.permute(0,2,3,1).reshape(27, C)), + then -.
 * C in {32, 64, 128, 256}; other widths return WMD_ERR_UNSUPPORTED (callers use the unfused operators).       */
typedef struct {
    int B, H, W, C;
    float slope;
    const float* x;      /* [B,C,H,W]      */
    const float* wp1;
    const float* bias1;
    const float* wp2;
    float* t;            /* [B,t_planes,H,W]  */
    int chain;           /* 0: the + and - chains -> t planes 0..53.
                            1: the coarsest level's low-pass chain (C -> C/4 -> 1, depth_decoder.py:104-106,126-129) as a
                               second launch over the same x: wp1 / bias1 = its [C/4, C, 1, 1] filter, wp2 = ONE
                               [27, C/4, 1, 1] image whose rows 0..8 hold the nine taps -> t planes 54..62 of an 81-plane t,
                               completed by wmd_head_shiftsum_fwd(yl_out).  C = 256 only (WMD_ERR_UNSUPPORTED otherwise)   */
    int t_planes;        /* planes per image of t: 0 or 54, or 81 when the low-pass chain shares the buffer              */
    /* optional [B,H,W] bytes (round 4, chain = 0 on the chained kernel): a run of pixels without a set byte is skipped (its
     * t planes are not written).  The sparse decoders pass the upconv1 mask = the 3x3 dilation of the wavelet mask: exactly
     * the pixels whose tap-partials a surviving output of wmd_head_shiftsum_fwd(yh_mask) gathers.                          */
    const uint8_t* run_mask;
    /* optional (round 4, chain = 0, C = 256, t_planes = 81): the low-pass chain's operands (what a chain = 1 call would take as
     * wp1 / bias1 / wp2).  The same call then fills planes 54..62 too -- on the chained kernel as a third group of workgroups
     * of the SAME launch (a quarter of a side's first product: an LL workgroup walks four pixel tiles, so the launch stays
     * inside one round of workgroup slots), otherwise as a second launch issued by the library.                            */
    const float* ll_wp1;
    const float* ll_bias1;
    const float* ll_wp2;
    /* optional (round 5, training forward on the fused kernels: trainer.py:208-212 needs what autograd would have kept): the
     * LeakyReLU outputs of the 1x1 stage are ALSO written to mid_out [B, mid_ct, H, W], channels mid_off_p.. (+ side),
     * mid_off_n.. (- side) and, with the low-pass chain riding along, mid_off_ll.. (C/4 channels) -- the layout the heads'
     * backward operators (wmd_head3x3_bwd / wmd_head1x1_bwd) read.  Chained kernel only (C = 64, 128, 256, chain = 0):
     * WMD_ERR_UNSUPPORTED otherwise.                                                                                      */
    float* mid_out;
    int mid_ct, mid_off_p, mid_off_n, mid_off_ll;
} wmd_head_fused_args;
int wmd_head_fused_fwd(const wmd_head_fused_args* args, void* stream);
/* Round 6: the first stage of up to three levels in ONE launch (chained widths 64 / 128 / 256, no run_mask / mid_out; anything else
 * falls back to n_levels calls of wmd_head_fused_fwd).  The heads of a level read only that level's trunk activation
 * (depth_decoder.py:126-136,164-166), so a dense decoder may postpone levels 4..2 until `upconv(2,1)` is done: alone none of them
 * fills 256 CUs, together they balance.  Same tap-partial planes, bit for bit.                                                  */
int wmd_head_fused_multi_fwd(const wmd_head_fused_args* levels, int n_levels, void* stream);

typedef struct {
    int B, H, W;
    int pad_mode;        /* padding of the 3x3 it completes (reflect for the KITTI heads)                    */
    float scale;         /* 2^(s-1)                                                                          */
    const float* t;      /* [B,54,H,W] from wmd_head_fused_fwd                                               */
    const float* bias_p; /* [3] */
    const float* bias_n; /* [3] */
    float* yh;           /* [B,3,H,W] = scale*sigmoid(.) - scale*sigmoid(.)                                  */
    /* optional fused IDWT (wmd_idwt_haar_fwd semantics): yl [B,H,W] -> out [B,2H,2W], disp                  */
    const float* yl;
    float* out;
    float* disp;
    float disp_scale;
    int clamp01;
    /* optional low-pass head completed in the same pass (t then has 81 planes per image, see wmd_head_fused_args.chain):
     * yl_out [B,H,W] = scale_ll * sigmoid(bias_ll[0] + nine shifted taps of planes 54..62); it is also the low-pass input
     * of the synthesis (yl must be NULL).                                                                                */
    const float* bias_ll; /* [1] or NULL */
    float scale_ll;
    float* yl_out;
    /* optional [B,H,W] bytes: yh is zeroed where the mask is 0 before it is stored and synthesised (the wavelet mask of the
     * sparse decoders' dense branch, depth_decoder.py:272)                                                              */
    const uint8_t* yh_mask;
    /* optional [B][2] uint32 (round 4): the order-preserving keys of the running (min, max) of every frame's `out` (the new
     * low-pass plane) are folded in with one atomic pair per wavefront -- the range the NEXT level's threshold needs
     * (depth_decoder.py:308: yl.max() - yl.min()) without a reduction pass of its own.  The key is csrc/wmd_internal.h's
     * order_key(f) = bits(f) ^ (sign ? 0xFFFFFFFF : 0x80000000), read back with order_unkey; armed state (0xFFFFFFFF, 0);
     * consumed by wmd_mask_level_lists.                                                                                  */
    uint32_t* range_keys;
    /* optional (round 5, training forward): the sigmoid outputs themselves -- sig_p, sig_n [B,3,H,W], sig_ll [B,1,H,W] (with
     * yl_out) -- whose s (1 - s) the backward of the heads multiplies by (what wmd_head3x3_fwd returns as sig_p / sig_n)      */
    float* sig_p;
    float* sig_n;
    float* sig_ll;
} wmd_head_shiftsum_args;
int wmd_head_shiftsum_fwd(const wmd_head_shiftsum_args* args, void* stream);
/* Round 5: the completions of up to three CONSECUTIVE levels (coarse to fine, each twice the size of the one before) in one launch --
 * level k's synthesis output is level k+1's low-pass input (depth_decoder.py:164: yl = IDWT((yl, [yh])) feeds the next iteration), so
 * levels[k > 0] carry yl = yl_out = NULL and take it from the chain; every level needs `out`.  Dense inference only (no yh_mask,
 * range_keys or sigmoid outputs).  Same values as n_levels calls of wmd_head_shiftsum_fwd.                                      */
int wmd_head_shiftsum_chain_fwd(const wmd_head_shiftsum_args* levels, int n_levels, void* stream);

/* Single-launch inference form of a level's two high-frequency heads AND the Haar synthesis that consumes them
 * (depth_decoder.py:108-136,164-166): 1x1 -> LeakyReLU -> 3x3 (as tap-partials) -> sigmoid -> 2^(s-1)(sig+ - sig-)
 * -> IDWT -> clamp, with every intermediate in LDS (wmd_head_level.hip).  Same operands as wmd_head_fused_fwd +
 * wmd_head_shiftsum_fwd, which remain the route for the widths this kernel does not cover.
 * wmd_head_level_supported(C) != 0 for C in {32, 64}.                                                            */
typedef struct {
    int B, H, W, C;
    int pad_mode;        /* padding of the 3x3 (reflect for the KITTI heads)                                  */
    float slope;         /* LeakyReLU slope of the 1x1 (0.1)                                                  */
    float scale;         /* 2^(s-1)                                                                           */
    const float* x;      /* [B,C,H,W]                                                                         */
    const float* wp1;    /* packed stacked [2C,C,1,1] filter, + rows first (wmd_conv_pack_weights)            */
    const float* bias1;  /* [2C] or NULL                                                                      */
    const float* wp2;    /* two packed [27,C,1,1] images (row co*9+tap), + then -                             */
    const float* bias_p; /* [3] or NULL                                                                       */
    const float* bias_n; /* [3] or NULL                                                                       */
    float* yh;           /* [B,3,H,W]                                                                         */
    const float* yl;     /* optional [B,H,W]: fused wmd_idwt_haar_fwd                                         */
    float* out;          /* [B,2H,2W] (with yl)                                                               */
    float* disp;         /* optional [B,2H,2W] = clamp(out * disp_scale)                                      */
    float disp_scale;
    int clamp01;
    const uint8_t* yh_mask; /* optional [B,H,W] bytes, see wmd_head_shiftsum_args.yh_mask                    */
    /* optional (round 5, training forward): the LeakyReLU outputs of the 1x1 stage -> mid_out [B, mid_ct, H, W] at channels
     * mid_off_p.. / mid_off_n.. (see wmd_head_fused_args.mid_out) and the sigmoid outputs sig_p, sig_n [B,3,H,W]             */
    float* mid_out;
    int mid_ct, mid_off_p, mid_off_n;
    float* sig_p;
    float* sig_n;
} wmd_head_level_args;
int wmd_head_level_supported(int C);
int wmd_head_level_fwd(const wmd_head_level_args* args, void* stream);
/* Round 6: the level's heads + synthesis AND the completions of up to three coarser levels in ONE launch (the streaming kernel's
 * pyramid, wmd_head_stream.hip): coarse[k] as for wmd_head_shiftsum_chain_fwd (coarse to fine; the finest is half this level's size
 * and its synthesis output IS this level's low-pass input, depth_decoder.py:164: args->yl must be NULL).  Same values, bit for bit,
 * as wmd_head_shiftsum_chain_fwd followed by wmd_head_level_fwd.  Dense inference outputs only; C = 32, H and W multiples of 8.    */
int wmd_head_level_pyramid_supported(int C, int B, int H, int W);   /* 0: no; 1: runs; 2: runs and is expected to pay (enough CUs for its <= 64-row segments) */
int wmd_head_level_pyramid_fwd(const wmd_head_level_args* args, const wmd_head_shiftsum_args* coarse, int n_coarse, void* stream);

/* Backward of the 3x3 stage of a level's wavelet heads (training): the 2-3 heads Conv3x3(C, 3 | 1) + sigmoid of a level
 * (depth_decoder.py:104-136; backward from torch.autograd, KITTI/trainer.py:211) given the pre-sigmoid gradients dy3
 * [B,n_out,H,W] (rows [LL], +, -) and the LeakyReLU outputs mid [B,Ct,H,W] of the stacked 1x1 stage:
 *   dzmid = act'(mid) * conv3x3^T(dy3)  (the 1x1 stage's pre-activation gradient),  dw3 / db3 per head.
 * One pass each over mid for the data and the weight gradient, no padded-domain buffer (wmd_head_bwd.hip).  At most 24
 * 64-channel slices over all heads (WMD_ERR_UNSUPPORTED beyond: use wmd_conv_dgrad / wmd_conv_wgrad on the stacked filter).
 * Alignment: when H*W is a multiple of 4 the planes of mid and dzmid are read and written sixteen bytes at a time, so both
 * pointers must be 16-byte aligned (any float pointer otherwise); the workspace always.  WMD_ERR_BAD_ARG if not: the last refusal
 * before a launch, after the workspace's size (the query answers for any pointers).                                         */
typedef struct {
    int row0;          /* first plane of dy3 that belongs to this head                   */
    int nrows;         /* its output channels: 3 (high-frequency heads) or 1 (low-pass)  */
    int ch0;           /* first channel of mid that belongs to this head                 */
    int nch;           /* its channel count                                              */
    const float* w3;   /* [nrows, nch, 3, 3]                                             */
    float* dw3;        /* [nrows, nch, 3, 3]                                             */
    float* db3;        /* [nrows]                                                        */
} wmd_head_bwd_head;
typedef struct {
    int B, H, W;
    int Ct;            /* channels of mid                                                */
    int n_out;         /* planes of dy3                                                  */
    int pad_mode;      /* padding of the 3x3 (reflect for the KITTI heads)               */
    int act;           /* activation that produced mid: WMD_ACT_LEAKY (or NONE / ELU)    */
    float slope;
    const float* dy3;  /* [B,n_out,H,W]                                                  */
    const float* mid;  /* [B,Ct,H,W]                                                     */
    float* dzmid;      /* [B,Ct,H,W]; channels of no head are not written                */
    int n_heads;       /* 1..3                                                           */
    wmd_head_bwd_head head[3];
    float* workspace;  /* wmd_head3x3_bwd_workspace_floats(args) floats                  */
    size_t workspace_floats;
} wmd_head3x3_bwd_args;
size_t wmd_head3x3_bwd_workspace_floats(const wmd_head3x3_bwd_args* args);
int wmd_head3x3_bwd(const wmd_head3x3_bwd_args* args, void* stream);

/* Backward of the 1x1 stage of a level's wavelet heads (training): the first layers Conv1x1(C, C | C/4) of every head of a
 * level, stacked along the output channels (depth_decoder.py:104-136), given the pre-activation gradient dz [B,Ct,H,W] of the
 * stack (wmd_head3x3_bwd's dzmid):  dx = act_x'(x) * w1^T dz (optional),  dw1 = sum_p dz (x) x,  db1 = sum_p dz.
 * One pass over dz and x each for the data and the weight gradient (wmd_head_bwd1.hip).
 * Alignment: when H*W is a multiple of 4, dz, x and dx (if given) must be 16-byte aligned (16-byte loads and stores of their
 * planes); the workspace always.  WMD_ERR_BAD_ARG if not: the last refusal before a launch, after the workspace's size.      */
typedef struct {
    int B, H, W;
    int C;             /* channels of x                                                  */
    int Ct;            /* channels of dz = rows of w1 (a multiple of 8)                  */
    int x_act;         /* activation that produced x (WMD_ACT_ELU for the decoders' trunk; NONE: no gate) */
    float x_slope;
    const float* dz;   /* [B,Ct,H,W]                                                     */
    const float* x;    /* [B,C,H,W]                                                      */
    const float* w1;   /* [Ct,C] (the [Ct,C,1,1] filters of the heads, concatenated)     */
    float* dx;         /* [B,C,H,W] or NULL                                              */
    float* dw1;        /* [Ct,C]                                                         */
    float* db1;        /* [Ct]                                                           */
    float* workspace;  /* wmd_head1x1_bwd_workspace_floats(args) floats                  */
    size_t workspace_floats;
} wmd_head1x1_bwd_args;
size_t wmd_head1x1_bwd_workspace_floats(const wmd_head1x1_bwd_args* args);
int wmd_head1x1_bwd(const wmd_head1x1_bwd_args* args, void* stream);
/* Both stages of a level's high-frequency heads in three launches instead of six: the 3x3 data gradient (-> dzmid); then the
 * 3x3 weight gradient, the 1x1 data gradient and the 1x1 weight gradient -- independent of each other once dzmid exists, each a
 * latency chain on its own -- as ONE launch; then both reduces as one.  Same arguments and results as wmd_head3x3_bwd(a3)
 * followed by wmd_head1x1_bwd(a1) with a1->dz == a3->dzmid; 3-channel heads only (a level with the low-pass head: the two
 * separate calls).  Round 6: a level of two 32-channel heads over a 32-channel x (Ct = 64, whole 64-pixel tiles, W % 4 == 0,
 * dx wanted) runs all four GEMMs as ONE launch (head_bwd_fused32_kernel) + the reduce; dzmid then stays in LDS and the buffer
 * is NOT written (it is scratch of this call either way).  WMD_HEAD_BWD_FUSED=0: always the three-launch form.               */
int wmd_head_bwd(const wmd_head3x3_bwd_args* a3, const wmd_head1x1_bwd_args* a1, void* stream);

/* ------------------------------------------------------------------ *
 * Sparse (threshold-gated) decoder path, batch 1
 *
 * Layout decision: activations stay DENSE [C,H,W] (zero-initialised by the caller); sparsity lives in
 *   - uint8 masks [H,W] (the reference's lowres/upconv0/upsample/upconv1/wavelet masks), and
 *   - compacted raster-order lists of active pixel indices (y*W+x) with a device-side count,
 * so no kernel needs a host-visible nnz and no index map is ever materialised.  The reference's
 * compact-tensor semantics are kept exactly: a neighbour that is not in the input mask reads 0
 * (KITTI/layers.py:439-453), index-map padding becomes coordinate padding followed by the mask test.
 * ------------------------------------------------------------------ */

/* out2[0] = min(x), out2[1] = max(x)   (depth_decoder.py:308 `yl.max() - yl.min()`), n >= 1. */
int wmd_minmax(const float* x, size_t n, float* out2, void* stream);

/* mask[p] = (max_b |yh[b,p]| > (minmax[1]-minmax[0]) * thresh_ratio) ? 1 : 0   (depth_decoder.py:308-309).
 * yh [3,h,w] planes.  The comparison is done exactly as the reference does it in fp32.            */
int wmd_mask_threshold(const float* yh, const float* minmax, float thresh_ratio, uint8_t* mask,
                       int h, int w, void* stream);

typedef struct {
    int up;          /* 1 or 2: nearest-upsample the input mask first (depth_decoder.py:311)       */
    int radius;      /* 0,1,2 ...: MaxPool2d(2r+1, stride 1, padding r) (:313-319)                 */
    uint8_t* out;    /* [h*up, w*up]                                                               */
    int32_t* nnz;    /* optional: the number of set pixels of frame f is ADDED to nnz[f * nnz_stride] (the caller
                        zero-initialises it) -- the pixel count of a mask without a compaction pass               */
    int nnz_stride;
} wmd_dilate_spec;
/* All dilated variants of one mask in a single launch (n <= 8). */
int wmd_mask_dilate_multi(const uint8_t* mask, int h, int w, const wmd_dilate_spec* specs, int n, void* stream);
/* Batched forms (extension: the reference's sparse decoder asserts batch 1, depth_decoder.py:297; on a 256-CU GPU one
 * 640x192 frame cannot fill the machine, so B frames -- each with its own range, threshold mask, pixel lists and counts --
 * go through the SAME launches): mask [B,h,w], every specs[i].out [B,h*up,w*up].                                        */
int wmd_mask_dilate_multi_b(const uint8_t* mask, int B, int h, int w, const wmd_dilate_spec* specs, int n, void* stream);

/* wmd_minmax + wmd_mask_threshold + wmd_mask_dilate_multi of one decoder level in ONE launch
 * (depth_decoder.py:308-319): thr = (max(yl) - min(yl)) * thresh_ratio over yl[n_yl]; base[p] = max_b |yh[b,p]| > thr
 * on the [h,w] grid of yh [3,h,w]; specs[i].out = dilation of the (nearest-upsampled) base mask exactly as
 * wmd_mask_dilate_multi would produce it; a spec (up 1, radius 0) yields the base mask itself.  Bit-identical to the
 * three separate calls (min/max are order-independent, the threshold is the same fp32 expression).          */
int wmd_mask_level(const float* yl, size_t n_yl, const float* yh, float thresh_ratio, int h, int w,
                   const wmd_dilate_spec* specs, int n, void* stream);
/* batched: yl [B,n_yl], yh [B,3,h,w], outputs [B,...]; the range (max - min) is taken per frame.  minmax_scratch: optional
 * [B,2] device floats -- with it the ranges come from one extra launch instead of a whole-plane reduction in every block */
int wmd_mask_level_b(const float* yl, size_t n_yl, const float* yh, float thresh_ratio, int B, int h, int w,
                     const wmd_dilate_spec* specs, int n, float* minmax_scratch, void* stream);

/* ---- Work-list form of a sparse level's mask launch (round 4) --------------------------------------------------------
 * One launch per decoder level, as wmd_mask_level_b / wmd_mask_dilate_multi_b, that ALSO
 *   * compacts, per spec that asks for it, the pixel tiles (tile_h x tile_w) holding at least one set pixel into a work
 *     list for wmd_conv_args.out_tiles: every workgroup finds the active tiles of its own 16x16-cell region (a bit per
 *     tile: wavefront OR-reduction + popcount = the offsets inside its run) and reserves a run of the list with one atomic;
 *     the frame's last workgroup (ticket counter) publishes the frame's total.  List order is unspecified, values never depend
 *     on it.  Tile shapes must nest in the region: tile_h, tile_w divide 16 * up, at most 32 tiles per region.
 *   * publishes the per-frame pixel counts of the specs that ask for it WITHOUT a zero-initialised accumulator of the
 *     caller's and without a copy: accumulators live in `scratch` (all zero at rest: the last workgroup moves them out and
 *     re-arms them) and are written to slot (seq % ring_slots) of the int32 ring `counts` [ring_slots][slot_ints] at
 *     [1 + counts_off + frame * ncounts + (count - 1)]; seq is a launch counter kept in scratch and advanced by the launch
 *     that has `advance` set (the last mask launch of a decoder forward), which also stamps slot[0] = seq + 1 -- so a host
 *     that counts its forwards the same way can fetch the counts of forward k from slot k % ring_slots whenever it wants
 *     them (and verify the stamp), and a forward that nobody asks pays neither a fill, nor a copy, nor a sync.
 *   * takes the LL range from `range_keys` when given: [B][2] order_key uint32 keys of (min, max) that the head
 *     kernels' epilogues maintain with atomics (wmd_head_shiftsum_args.range_keys); consumed and re-armed
 *     (0xFFFFFFFF, 0) by this launch.  Else `minmax` [B,2] floats, else every block reduces yl itself.
 * scratch: wmd_mask_level_scratch_ints(B) int32, zero-initialised ONCE by the caller, private to one stream.            */
typedef struct {
    int up, radius;        /* as wmd_dilate_spec                                                                      */
    uint8_t* out;          /* [B, h*up, w*up]                                                                         */
    int count;             /* k > 0: this spec's pixel count is published as count column k - 1 (k <= ncounts <= 8)    */
    int tile_h, tile_w;    /* != 0: build the active-tile list of this spec's mask                                     */
    int32_t* tile_list;    /* [B][ceil(h*up / tile_h) * ceil(w*up / tile_w)]: frame f's tiles fill the head of its segment */
    int32_t* tile_count;   /* [B], overwritten                                                                         */
    const uint8_t* and_mask; /* optional [B, h*up, w*up]: out = dilation AND and_mask.  The never-refilled activation planes
                              of the work-list form hold stale values outside the previous level's support; the reference
                              reads 0 there (sparse_select, KITTI/layers.py:392-400: a pixel absent from the previous index
                              map gathers the prepended zero), so the input mask of upconv(i,0) is lowres AND the previous
                              level's upconv1 mask -- a no-op for thresholded masks, which are nested by construction   */
} wmd_level_spec;

typedef struct {
    int B, h, w;
    const float* yl;       /* [B, n_yl]   threshold form (depth_decoder.py:308-309) ...                                */
    size_t n_yl;
    const float* yh;       /* [B, 3, h, w]                                                                            */
    float thresh_ratio;
    const uint8_t* mask0;  /* ... or an injected base mask [B, h, w] (yl / yh unused)                                  */
    const float* minmax;   /* optional [B, 2]                                                                          */
    uint32_t* range_keys;  /* optional [B, 2], see above                                                               */
    const wmd_level_spec* specs;
    int n;                 /* <= 8                                                                                     */
    int32_t* scratch;
    int32_t* counts;       /* the ring (NULL when ncounts == 0)                                                        */
    int ring_slots, slot_ints, counts_off, ncounts;
    int advance;
} wmd_mask_level_args;
size_t wmd_mask_level_scratch_ints(int B);
int wmd_mask_level_lists(const wmd_mask_level_args* args, void* stream);

typedef struct {
    const uint8_t* mask;   /* [npix]                                                               */
    int npix;
    int32_t* coords;       /* [npix] capacity; receives the active pixel indices in raster order   */
    int32_t* nnz;          /* device scalar                                                        */
} wmd_compact_spec;
/* Stream compaction (mask2idxmap / mask2yx, KITTI/layers.py:371-389) of up to 8 masks in one launch:
 * one workgroup per mask; a lane packs 16 flags into a bit field (popcount), wavefront shuffle prefix sums + an LDS scan
 * over the 16 wavefronts, raster order preserved.                                                   */
int wmd_mask_compact_multi(const wmd_compact_spec* specs, int n, void* stream);
/* batched: specs[i].mask / .coords are [B,npix]; specs[i].nnz points at the count of (frame 0, mask i) of an int32 [B,n]
 * array (the counts of one frame are contiguous)                                                                      */
int wmd_mask_compact_multi_b(const wmd_compact_spec* specs, int n, int B, void* stream);

typedef struct {
    int H, W;              /* output resolution                                                    */
    int C1, up1;           /* source 1: dense [C1tot, H/up1, W/up1]; channels [c1_off, c1_off+C1) used */
    int C1tot, c1_off;
    int C2;                /* source 2 (skip): dense [C2,H,W]; 0 if none                           */
    int Cout, ksize, pad_mode, act;
    float slope;
    const float* x1;
    const float* x2;
    const uint8_t* in_mask;      /* [H,W] support of the virtual input; NULL = everywhere          */
    const int32_t* out_coords;   /* active output pixels                                          */
    const int32_t* out_nnz;
    int max_out;                 /* launch bound: capacity of out_coords                          */
    const float* wp;             /* packed weights [Cout, C1+C2, k, k] (wmd_conv_pack_weights)     */
    const float* bias;
    /* dual-head mode (wp2 != NULL, Cout <= 16): a second filter over channels [c1_off2, c1_off2+C1)
     * of x1; y = out_scale*act(conv) - out_scale*act(conv2)   (depth_decoder.py:276-290)          */
    const float* wp2;
    const float* bias2;
    int c1_off2;
    float out_scale;             /* y = out_scale * act(conv + bias)                              */
    float* y;                    /* dense [Cout,H,W]; written at the active pixels only            */
    int split_waves;             /* 0 = default (2048).  The wavefronts of a block split the input channels of one
                                  * 16-pixel tile while (tiles x slices) stays below this count, and take longer
                                  * channel ranges of separate tiles beyond it (decided on the device from *out_nnz);
                                  * 1 = never split, INT_MAX = always split.  Results agree to fp32 rounding.      */
    int B;                       /* frames decoded by this launch (0 or 1: one).  x1 [B,C1tot,..], x2 [B,C2,H,W], in_mask
                                  * [B,H,W], out_coords [B,max_out], y [B,Cout,H,W]; weights are shared               */
    int nnz_stride;              /* int32 elements between the counts of consecutive frames (out_nnz + b*nnz_stride)  */
} wmd_sparse_conv_args;

/* Gather-GEMM convolution on the active pixels (sparse_conv3x3 / sparse_conv1x1 / sparse_upsample /
 * sparse_select, KITTI/layers.py:337-507) on fp32 MFMA: one wavefront = 16 active pixels x up to 64
 * output channels; the B operand is gathered per lane through the coordinate-padding + mask test.  */
int wmd_sparse_conv(const wmd_sparse_conv_args* args, void* stream);

/* The table of instantiations behind wmd_sparse_conv: wmd_sparse_conv_config_name returns e.g.
 * "sparse_conv_kernel<2,9,false,8,2,true>" (the kernel's template arguments MR,TAPS,DUAL,WK,UN,ROWS: the name the launch
 * profile shows) or NULL when i is out of range.                                                                        */
int wmd_sparse_conv_num_configs(void);
const char* wmd_sparse_conv_config_name(int i);

/* What wmd_sparse_conv would launch on this problem (host code: no HIP call, no pointer is dereferenced; wp2 != NULL is read
 * as "dual-head mode" and nothing else): the table index of the instantiation, *grid_x (may be NULL) receives the launch's
 * grid.x.  -1 with wmd_last_error() set to wmd_sparse_conv's own text for a problem that entry refuses (its null-pointer tests
 * on the tensors aside); -1 with *grid_x = 0 and no error for max_out = 0, where wmd_sparse_conv launches nothing.           */
int wmd_sparse_conv_plan(const wmd_sparse_conv_args* args, int* grid_x);

/* ------------------------------------------------------------------ *
 * Multi-scale loss front-end
 * ------------------------------------------------------------------ */
/* F.interpolate(x, [H,W], mode="bilinear", align_corners) (KITTI/trainer.py:337-338 with align_corners=False;
 * NYUv2/train.py:304-305 with align_corners=True, H = h*2^s) and, when depth != NULL, disp_to_depth
 * (KITTI/layers.py:16-25): depth = 1 / (1/max_depth + (1/min_depth - 1/max_depth) * y).
 * x [N,h,w] -> y [N,H,W] (may be NULL), depth [N,H,W] (may be NULL).                                        */
int wmd_upsample_bilinear_fwd(const float* x, float* y, float* depth, int N, int h, int w, int H, int W,
                              int align_corners, float min_depth, float max_depth, void* stream);
/* Adjoint: dx [N,h,w] = B^T (dy + ddepth * d depth/d y); `depth` is the forward output (needed with ddepth). */
int wmd_upsample_bilinear_bwd(const float* dy, const float* ddepth, const float* depth, float* dx, int N, int h,
                              int w, int H, int W, int align_corners, float min_depth, float max_depth, void* stream);

/* ------------------------------------------------------------------ *
 * Data-parallel gradient exchange (new: the reference is single-GPU, trainer.py:45)
 * ------------------------------------------------------------------ */
typedef struct wmd_comm wmd_comm;
/* unique_id: 128 bytes produced by rank 0 with wmd_comm_unique_id and broadcast by the caller */
int wmd_comm_unique_id(void* unique_id_128);
int wmd_comm_init(wmd_comm** comm, const void* unique_id_128, int world, int rank);
/* in-place sum all-reduce of `n` floats then scale by `scale` (1/world), on `stream` */
int wmd_comm_allreduce(wmd_comm* comm, float* buf, size_t n, float scale, void* stream);
/* in-place broadcast of n floats from rank `root` (initial parameter / BatchNorm-buffer synchronisation of the replicas) */
int wmd_comm_broadcast(wmd_comm* comm, float* buf, size_t n, int root, void* stream);
/* what the communicator itself reports: the RCCL version code (ncclGetVersion), ncclCommCount, ncclCommUserRank */
int wmd_comm_info(wmd_comm* comm, int* rccl_version, int* world, int* rank);
int wmd_comm_destroy(wmd_comm* comm);

/* ------------------------------------------------------------------ *
 * Evaluation arithmetic behind the reference's accuracy claims; batches stay in HBM.
 * ------------------------------------------------------------------ */

/* Per-image chain of KITTI/evaluate_depth.py:268-307 for B images of one size:
 *   pred_disp [B,h,w] --cv2.resize (bilinear, half-pixel centres, edge clamp)--> [B,H,W] --> depth = pred_scale / disp
 *   mask_mode 1: Eigen split: min_depth < gt < max_depth inside the Garg crop (:284-290); 0: gt > 0 (:293)
 *   median_scaling != 0: depth *= median(gt[mask]) / median(depth[mask])  (:298-301; np.median = mean of the two middle values)
 *   depth = clamp(depth, min_depth, max_depth) (:304-305); compute_errors (:50-68)
 * out [B,9] = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, log10, n_valid  (a row of NaN + 0 when the mask is empty);
 * the applied ratio of image b is left in workspace (see wmd_eval_workspace_floats) for the caller to read.        */
typedef struct {
    int B, h, w, H, W;
    float min_depth, max_depth;   /* 1e-3, 80 (evaluate_depth.py:85-86)                    */
    int mask_mode;
    float pred_scale;             /* pred_depth_scale_factor (5.4 for stereo, :35)         */
    int median_scaling;
    const float* pred_disp;
    const float* gt_depth;
    float* out;
    float* workspace;             /* wmd_eval_workspace_floats(B, H, W)                    */
    size_t workspace_floats;
} wmd_eval_kitti_args;
/* Floats of workspace (0 for a size < 1).  What the caller may read after the call is the prefix, in floats: two [B,H,W] planes (the
 * resized depth and the ground truth, -1 outside the mask), [B] valid-pixel counts (int32), [B,2] medians (depth, ground truth: with median_scaling the
 * applied ratio of image b is the second over the first, at float 2 B H W + B + 2 b).  What follows belongs to the library.
 * NULL is WMD_ERR_BAD_ARG, a short workspace WMD_ERR_WORKSPACE; any float pointer is aligned enough.                             */
size_t wmd_eval_workspace_floats(int B, int H, int W);
int wmd_eval_kitti(const wmd_eval_kitti_args* args, void* stream);

/* compute_errors (KITTI/evaluate_depth.py:50-68) and compute_errors_nyu (NYUv2/utils.py:85-98) on B prepared
 * arrays of n_per_image positive values each: out9 [B,9] as above (NYUv2 reads abs_rel, rmse, log10, a1..a3).
 * Entries with gt < 0 are skipped (masked).                                                                      */
int wmd_eval_errors(const float* pred, const float* gt, int B, size_t n_per_image, float* out9, void* stream);

/* batch_post_process_disparity (KITTI/evaluate_depth.py:71-79) with the [:, :, ::-1] flip of the second operand
 * (:204) fused: r_disp is the raw prediction for the mirrored image.  l_disp, r_disp, out: [B,h,w].              */
int wmd_flip_postprocess(const float* l_disp, const float* r_disp, float* out, int B, int h, int w, void* stream);

/* Depth-boundary errors of the NYUv2 evaluation: compute_depth_boundary_error (NYUv2/utils.py:122-169), the dbe_acc /
 * dbe_com columns of NYUv2/evaluate.py:94-107, for B images of H x W in one call; nothing is read back to the host.
 *
 * wmd_eval_canny: img [B,H,W] float -> edges_u8 [B,H,W] (0 / 1).  This is the project's own definition of the detector,
 * modelled on skimage.feature.canny(image, sigma, low, high) with mask=None (agreement with an actual skimage is not
 * verified); all arithmetic is float64:
 *   smoothed = G(img) / (G(ones) + 2.220446049250313e-16), G the separable Gaussian of radius int(4 sigma + 0.5) with
 *              zeros outside the image (scipy.ndimage.gaussian_filter(mode="constant", truncate=4));
 *   isobel / jsobel = the Sobel derivatives along rows / columns with mirrored borders (d c b a | a b c d);
 *   mag = hypot(isobel, jsobel); a pixel off the one-pixel border ring with mag >= low survives when both neighbours along
 *   the gradient, interpolated between the two nearest of the eight neighbours, are <= mag;
 *   edges = the 8-connected components of the survivors that hold a survivor with mag >= high.
 * NaN follows IEEE rules: it spreads through the Gaussian and the Sobel window and fails every comparison.
 *
 * wmd_eval_dbe: pred [B,H,W] float, edges_gt_u8 [B,H,W] (non-zero = edge), mask_u8 [B,H,W] or NULL (all ones) ->
 * out2 [B,2] = (dbe_acc, dbe_com) and, unless NULL, edges_est_u8 [B,H,W]:
 *   p = pred in float64 with 0 -> NaN, p -= nanmin, p /= nanmax (a constant map is NaN everywhere: no edges);
 *   edges_est = the detector on p with sigma = sqrt(2) and the two thresholds;
 *   D_gt, D_est = exact Euclidean distances to the nearest edge pixel; F = edges_est (D_gt < 10) mask;
 *   F empty: (10, 10); else dbe_acc = sum(D_gt F) / sum(F),
 *   dbe_com = (sum(min(D_gt mask, 10) edges_est) + sum(min(D_est, 10) edges_gt)) / (sum(edges_est) + sum(edges_gt)).
 *   An image without ground-truth edges scores (NaN, NaN) with an empty edge map.
 * The sums are integer histograms over the squared distance added in a fixed order: the same input gives the same bits.
 *
 * Sizes: H, W >= 3 (WMD_ERR_BAD_SHAPE below); H * 2 * ceil(W / 64) <= 16384 -- the hysteresis keeps two bit planes of an
 * image in LDS; 480 x 640 needs 9600 -- and a radius of at most 12 taps (sigma <= 3.1): WMD_ERR_UNSUPPORTED beyond, before
 * any launch.  workspace: wmd_eval_dbe_workspace_bytes(B, H, W) bytes, 8-byte aligned (0 for a bad shape): 832 B of state,
 * 8 H W of smoothed image and three bit planes of 4 H * 2 ceil(W / 64) per image.  A short one is WMD_ERR_WORKSPACE, then a
 * misaligned one WMD_ERR_BAD_ARG (as a NULL one), before any HIP call.                                                */
size_t wmd_eval_dbe_workspace_bytes(int B, int H, int W);
int wmd_eval_canny(const float* img, unsigned char* edges_u8, int B, int H, int W, double sigma, double low, double high,
                   void* workspace, size_t workspace_bytes, void* stream);
int wmd_eval_dbe(const float* pred, const unsigned char* edges_gt_u8, const unsigned char* mask_u8, float* out2,
                 unsigned char* edges_est_u8, int B, int H, int W, double low, double high, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * Photometric loss stack of the KITTI trainer, forward and backward
 * ------------------------------------------------------------------ */

/* SSIM (KITTI/layers.py:281-311) and compute_reprojection_loss (KITTI/trainer.py:393-405).  x = pred, y = target, [B,C,H,W].
 * mode 0: out [B,C,H,W] = clamp((1 - SSIM(x, y)) / 2, 0, 1)                      (the SSIM module)
 * mode 1: out [B,1,H,W] = w_ssim * mean_c(mode 0) + w_l1 * mean_c |y - x|        (0.85 / 0.15 in the trainer)
 * Backward: g has the shape of out; dx and/or dy [B,C,H,W] (either may be NULL); workspace = 3*B*C*H*W floats.       */
int wmd_ssim_fwd(const float* x, const float* y, float* out, int B, int C, int H, int W, int mode, float w_ssim, float w_l1,
                 void* stream);
size_t wmd_ssim_bwd_workspace_floats(int B, int C, int H, int W);
int wmd_ssim_bwd(const float* x, const float* y, const float* g, float* dx, float* dy, int B, int C, int H, int W, int mode,
                 float w_ssim, float w_l1, float* workspace, size_t workspace_floats, void* stream);

/* BackprojectDepth -> Project3D -> F.grid_sample(src, grid, padding_mode="border") (KITTI/layers.py:176-229,
 * KITTI/trainer.py:352-372) in one kernel: out[b,c,y,x] = bilinear(src[b,c], project(K T, depth[b,y,x] * inv_K (x,y,1))).
 * K, inv_K, T: [B,4,4] row-major.  Backward returns d(depth) [B,1,H,W] and dT [B,4,4]; the source frame and the
 * intrinsics are constants of the loss (no gradient), as in the trainer.                                              */
typedef struct {
    int B, C, H, W;      /* target grid = depth map size; C colour channels                                          */
    int Hs, Ws;          /* source frame size (equal to H, W in the trainer)                                         */
    float eps;           /* Project3D eps, 1e-7                                                                       */
    const float* src;    /* [B,C,Hs,Ws] */
    const float* depth;  /* [B,1,H,W]   */
    const float* K;
    const float* inv_K;
    const float* T;
} wmd_warp_args;
int wmd_warp_fwd(const wmd_warp_args* args, float* out, void* stream);
size_t wmd_warp_bwd_workspace_floats(const wmd_warp_args* args);
int wmd_warp_bwd(const wmd_warp_args* args, const float* grad_out, float* ddepth, float* dT, float* workspace,
                 size_t workspace_floats, void* stream);

/* get_smooth_loss (KITTI/layers.py:238-252): out[0] = mean |dx disp| exp(-gamma mean_c |dx img|) + the same along y.
 * disp [B,1,H,W], img [B,C,H,W]; backward w.r.t. disp only (grad_out: 1 float on the device).                          */
size_t wmd_smooth_workspace_floats(int B, int H, int W);
int wmd_smooth_fwd(const float* disp, const float* img, float* out, int B, int C, int H, int W, float gamma, float* workspace,
                   size_t workspace_floats, void* stream);
int wmd_smooth_bwd(const float* disp, const float* img, const float* grad_out, float* ddisp, int B, int C, int H, int W,
                   float gamma, void* stream);

/* Depth-hint fusion (KITTI/precompute_depth_hints.py:243-249; the disparity conversion of :149): per pixel, the depth of
 * the candidate whose reprojection of the other stereo view matches the base image best.  One launch, no M-fold copies.
 * The stereo matcher that produces the candidates is out of scope: they come from the caller.
 *   cand [B,M,H,W]: depths, or -- cand_is_disparity != 0 -- pixel disparities d, converted as
 *                   depth = focal_times_baseline / (d + 1e-7f) * (d > 0 ? 1 : 0).  A depth of 0 ("no match") is a legal
 *                   candidate and takes part in the minimum like any other, as in the reference.
 *   base, lookup [B,C,H,W] (C in 1..3, base in [0,1]); K, inv_K, T [B,4,4] row-major; T per image (the sign of the
 *                   baseline differs between a left and a right base image).
 *   loss(b,m,p) = w_ssim * mean_c clamp((1 - SSIM)/2, 0, 1) + w_l1 * mean_c |base - warped_m|, 3 x 3 windows over a
 *                   ReflectionPad2d(1) of both images, warped_m = wmd_warp_fwd's arithmetic on lookup with candidate m (the
 *                   reflected neighbour is the warped value at the reflected pixel, with that pixel's own candidate).
 *   best_index [B,H,W] (int): the lowest m among the smallest float32 losses (a running minimum with strict <);
 *   best_depth [B,1,H,W]: that candidate's depth, bit for bit the value that was warped; losses [B,M,H,W] or NULL: the
 *                   float32 values that were compared.
 * Refused before any HIP call: a NULL required pointer (WMD_ERR_BAD_ARG); B < 1, M < 1, C < 1, H < 2 or W < 2
 * (WMD_ERR_BAD_SHAPE); M > WMD_DEPTH_HINTS_MAX_CANDIDATES, C > 3, B > 65535, more than 2^31 elements
 * (WMD_ERR_UNSUPPORTED); workspace_floats below wmd_depth_hints_workspace_floats(B, M, H, W), or a non-zero
 * workspace_floats with a NULL workspace (WMD_ERR_WORKSPACE).  The kernel stages nothing in device memory, so the size
 * asked for is 0 today and NULL / 0 is accepted.  Finite inputs give finite losses (the SSIM denominators are >= C1 C2);
 * the result for non-finite inputs is undefined (no fault: a NaN sample coordinate reads pixel 0).                        */
#define WMD_DEPTH_HINTS_MAX_CANDIDATES 64
size_t wmd_depth_hints_workspace_floats(int B, int M, int H, int W);
int wmd_depth_hints_fuse(const float* cand, int cand_is_disparity, float focal_times_baseline, const float* base,
                         const float* lookup, const float* K, const float* inv_K, const float* T, float* best_depth,
                         int* best_index, float* losses, int B, int M, int C, int H, int W, float eps, float w_ssim, float w_l1,
                         float* workspace, size_t workspace_floats, void* stream);

/* KITTI ground-truth depth maps from velodyne scans: generate_depth_map (KITTI/kitti_utils.py:52-104) for B scans in one
 * call, nothing read back to the host.
 *   points  [total_points,4] float32, the scans packed one after the other in file order (x forward, y left, z up; the 4th
 *           column is ignored and taken as 1), 16-byte aligned; NULL only with total_points == 0
 *   offsets [B+1] int64 on the device: scan b is rows offsets[b] .. offsets[b+1]-1.  total_points is the host's length of
 *           the packed list (the offsets are not read back): no row at or beyond it is read, and a row that no scan claims
 *           is dropped
 *   P       [B,3,4] float64 row-major, the reference's P_velo2im per scan;  depth [B,H,W] float32
 * Per scan, with i the row's index in its scan:
 *   1. row i is kept iff x >= 0 (true for -0.0, false for NaN);
 *   2. in float64, every product and sum rounded on its own: p_r = ((P[r,0] x + P[r,1] y) + P[r,2] z) + P[r,3];
 *      u = rint(p_0 / p_2) - 1, v = rint(p_1 / p_2) - 1 (half to even, IEEE division, p_2 <= 0 not special-cased);
 *      val = x if vel_depth else p_2;
 *   3. the row is valid iff u >= 0, v >= 0, u < W and v < H, compared in float64;
 *   4. depth[v,u] = val of the valid row with the highest i at that pixel, 0 without one;
 *   5. key = v (W - 1) + u - 1 (the reference's sub2ind): for every key that more than one valid row holds, the pixel of
 *      that key's lowest-i row receives the minimum val over the key's rows;
 *   6. values < 0 become 0; val is rounded to float32 once (the minimum commutes with that rounding).
 * Rules 4 and 5 are resolved by integer atomics on packed (index, value) words: the same input gives the same bits.
 * The call initialises its workspace itself.  Three launches (two with total_points == 0).
 * Refused before any HIP call: a NULL offsets, P or depth, a NULL points with total_points > 0 or a misaligned
 * points (WMD_ERR_BAD_ARG); B, H or W < 1 (WMD_ERR_BAD_SHAPE); H W or total_points -- which bounds every
 * scan's length -- at or above 2^31 (WMD_ERR_UNSUPPORTED); a workspace that is NULL, not 8-byte aligned or shorter than
 * wmd_lidar_depth_workspace_bytes(B, H, W) (WMD_ERR_WORKSPACE).  The size query returns 0 for a shape the call refuses. */
size_t wmd_lidar_depth_workspace_bytes(int B, int H, int W);
int wmd_lidar_depth_maps(const float* points, const long long* offsets, const double* P, size_t total_points, int B, int H,
                         int W, int vel_depth, float* depth, void* workspace, size_t workspace_bytes, void* stream);

/* KITTI training inputs: MonoDataset.preprocess (KITTI/datasets/mono_dataset.py:118-145) for N decoded frames in one call,
 * bit for bit what the reference's chain gives over Pillow 12.2: flip, 8-bit Lanczos resize, ToTensor, ColorJitter.
 *
 * Tables (host only, no HIP call).  wmd_lanczos_ksize(in, out) and wmd_lanczos_table(in, out, ..) are wmd_resample_ksize and
 * wmd_resample_table (below) with WMD_FILTER_LANCZOS: the same tables, statuses and refusals under their own names.
 * wmd_color_pyramid_tables writes the tables of a whole pyramid, level after level as (bounds, coeffs) of the width then of
 * the height, wmd_color_pyramid_table_ints ints in all (0 for a shape the pyramid refuses); the caller uploads them once per
 * shape and passes the device copy as `tables`.
 *
 * wmd_color_pyramid.  frames [N,H0,W0,3] uint8 (HWC).  Level s in 0 .. num_scales-1 is h x w = (height >> s) x (width >> s),
 * resized from the uint8 level s-1 (level 0 from the frame): horizontal pass, uint8 intermediate, vertical pass, each
 * clip8(((1 << 21) + sum k[x] pix[xmin + x]) >> 22) in int32; an axis whose size does not change is copied.  flip [N] uint8 or
 * NULL: where set the frame is mirrored before level 0 (a mirrored gather in the first horizontal pass).  The three outputs
 * hold the levels one after the other, level s at pixel offset N (h_0 w_0 + .. + h_{s-1} w_{s-1}): levels uint8 [N,h,w,3],
 * color and color_aug float32 [N,3,h,w] = u8 / 255 (a float32 division).  enable [N] uint8, order [N,4] uint8 (a permutation
 * of 0 brightness, 1 contrast, 2 saturation, 3 hue; read & 3), factors [N,3] float32 (brightness, contrast, saturation),
 * hue_shift [N] int32 (read & 255), all on the device; enable == NULL: no jitter, color_aug may be NULL and is not written.
 * Where enable[n] is 0 color_aug equals color.  Otherwise each level's uint8 image goes through the four ops in order, each
 * uint8 -> uint8: blend(deg, img, f) = trunc(deg + f (img - deg)) in float32, product and sum rounded apart, clamped to
 * [0, 255] first unless 0 <= f <= 1; brightness deg = 0; saturation deg = grey = (19595 R + 38470 G + 7471 B + 0x8000) >> 16;
 * contrast deg = (2 sum grey + n) / (2 n) over the n pixels of that image as it enters the op; hue = Pillow's RGB -> HSV,
 * H = (H + hue_shift) & 255, HSV -> RGB.  The grey sums are 64-bit integer atomics: the same input gives the same bits.
 * Launches: one per level, one for ToTensor + jitter over all levels, and a memset of the workspace with jitter.
 * Refused before any HIP call: a NULL frames, tables, levels or color, jitter arrays given in part, enable without
 * color_aug (WMD_ERR_BAD_ARG); N, a size or num_scales < 1, num_scales > 8 or an empty last level (WMD_ERR_BAD_SHAPE); a
 * size above 32768, N above 65535 or a ratio whose row footprint does not fit the LDS (WMD_ERR_UNSUPPORTED); a workspace that
 * is NULL, not 8-byte aligned or shorter than wmd_color_pyramid_workspace_bytes (WMD_ERR_WORKSPACE; 0 for a refused shape).
 *
 * wmd_color_jitter: the jitter alone, images [N,h,w,3] uint8 -> out (same layout), a memset and two launches (grey sums, then the chain).
 * h w < 2^31.  wmd_color_jitter_workspace_bytes(N, h, w) = 8 N, 0 for a refused shape. */
int wmd_lanczos_ksize(int in, int out);
int wmd_lanczos_table(int in, int out, int* bounds, int* coeffs, int ksize);
size_t wmd_color_pyramid_table_ints(int H0, int W0, int height, int width, int num_scales);
int wmd_color_pyramid_tables(int H0, int W0, int height, int width, int num_scales, int* tables, size_t table_ints);
size_t wmd_color_pyramid_workspace_bytes(int N, int H0, int W0, int height, int width, int num_scales);
int wmd_color_pyramid(const unsigned char* frames, int N, int H0, int W0, int height, int width, int num_scales,
                      const unsigned char* flip, const unsigned char* enable, const unsigned char* order, const float* factors,
                      const int* hue_shift, const int* tables, unsigned char* levels, float* color, float* color_aug,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t wmd_color_jitter_workspace_bytes(int N, int h, int w);
int wmd_color_jitter(const unsigned char* images, unsigned char* out, int N, int h, int w, const unsigned char* enable,
                     const unsigned char* order, const float* factors, const int* hue_shift, void* workspace, size_t workspace_bytes,
                     void* stream);

/* NYUv2 training inputs: getDefaultTrainTransform / getNoTransform (NYUv2/data.py:22-68, :107-140, :199-214) and DepthNorm
 * (NYUv2/train.py:281) for B decoded samples in one call and ONE launch, bit for bit what the reference's chain gives over
 * Pillow 12.2: flip, channel swap, the gamma table, crop, 8-bit bicubic resize, ToTensor, * 1000 and the clamp.
 *
 * Tables (host only, no HIP call): Pillow's Resample.c precompute_coeffs + normalize_coeffs_8bpc, in double.  Per axis,
 * scale = in / out, fs = max(scale, 1), support = s fs with s = 2 for WMD_FILTER_BICUBIC and 3 for WMD_FILTER_LANCZOS,
 * ksize = ceil(support) 2 + 1 -- wmd_resample_ksize, 0 unless the filter is one of the two and 1 <= in, out <= 32768.  Per
 * output index xx: center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0),
 * n = min((int)(center + support + 0.5), in) - xmin, w[x] = f((x + xmin - center + 0.5) (1 / fs)) divided by their sum,
 * k[x] = (int)(w 2^22 +- 0.5), with f(t) = ((a + 2) |t| - (a + 3)) t^2 + 1 for |t| < 1, (((|t| - 5) |t| + 8) |t| - 4) a for
 * |t| < 2, a = -0.5 (bicubic) or f(t) = sinc(t) sinc(t / 3) on -3 <= t < 3 (Lanczos; libm sin).  wmd_resample_table writes
 * bounds [out][2] = (xmin, n) and coeffs [out][ksize], zero beyond n.  Refused: a NULL pointer, a filter that is neither, a
 * ksize that is not wmd_resample_ksize's (WMD_ERR_BAD_ARG); in or out outside 1..32768 (WMD_ERR_BAD_SHAPE).
 * wmd_nyu_inputs_tables writes the four bicubic tables of one call into `tables`, as (bounds, coeffs) of: image width
 * (W0 - 2 crop -> iw), image height (H0 - 2 crop -> ih), depth width (-> dw), depth height (-> dh);
 * wmd_nyu_inputs_table_ints ints in all (0 for a shape the call refuses).  The caller uploads them once per shape and passes
 * the device copy and its length.
 *
 * wmd_nyu_inputs.  image_u8 [B,H0,W0,3] and depth_u8 [B,H0,W0] uint8 on the device.  Per item b, in the reference's order:
 *   flip [B] uint8 or NULL: where set, image and depth are mirrored left-right (a mirrored source column);
 *   perm [B] uint8 or NULL: index into itertools.permutations(range(3)) = 012, 021, 102, 120, 201, 210 (read clamped to 5):
 *     image[..., k] = image[..., perm[k]];
 *   lut [B,256] uint8 or NULL: image = lut[b][image], every channel (the reference's gamma, built by the caller);
 *   the crop box (crop, crop, W0 - crop, H0 - crop) of both;
 *   resize of the image to ih x iw and of the depth map to dh x dw: horizontal pass, uint8 intermediate, vertical pass, each
 *     clip8(((1 << 21) + sum k[x] pix[xmin + x]) >> 22) in int32; an axis whose size does not change is copied;
 *   image [B,3,ih,iw] float32 = u8 / 255 (a float32 division); depth [B,1,dh,dw] float32 =
 *     min(max((u8 / 255) * 1000, 10), 1000), every operation rounded on its own; disp_gt (same shape) or NULL = 10 / depth;
 *   image_resized [B,ih,iw,3] and depth_resized [B,dh,dw] uint8 or NULL: the resized planes in front of the conversion.
 * A block owns 64 x th output pixels of one image or one depth map and stages their source footprint in LDS; th (at most 16)
 * is the largest power of two whose footprint, intermediate and coefficients fit 48 KiB.
 * Refused before any HIP call: a NULL image_u8, depth_u8, tables, image or depth, a misaligned tables, a table_ints that is
 * not wmd_nyu_inputs_table_ints of the shape (WMD_ERR_BAD_ARG); B or a size < 1, crop < 0, 2 crop >= H0 or 2 crop >= W0
 * (WMD_ERR_BAD_SHAPE); a size above 32768, B above 65535, or a ratio at which one output row's footprint does not fit the
 * LDS (WMD_ERR_UNSUPPORTED). */
typedef enum { WMD_FILTER_BICUBIC = 0, WMD_FILTER_LANCZOS = 1 } wmd_filter;
int wmd_resample_ksize(int filter, int in, int out);
int wmd_resample_table(int filter, int in, int out, int* bounds, int* coeffs, int ksize);
size_t wmd_nyu_inputs_table_ints(int H0, int W0, int crop, int ih, int iw, int dh, int dw);
int wmd_nyu_inputs_tables(int H0, int W0, int crop, int ih, int iw, int dh, int dw, int* tables, size_t table_ints);
int wmd_nyu_inputs(const unsigned char* image_u8, const unsigned char* depth_u8, int B, int H0, int W0, int crop, int ih, int iw,
                   int dh, int dw, const unsigned char* flip, const unsigned char* perm, const unsigned char* lut,
                   const int* tables, size_t table_ints, float* image, float* depth, float* disp_gt,
                   unsigned char* image_resized, unsigned char* depth_resized, void* stream);

/* ------------------------------------------------------------------ *
 * Colour images of the predictions (csrc/wmd_viz.hip)
 * ------------------------------------------------------------------ */

/* The three places the reference turns a map into a picture, for a batch in device memory, with the bytes numpy 2.2 and
 * matplotlib 3.10 give on the host.  Common to all three: `lut` is a device pointer to 768 bytes, 256 rows of (r, g, b) --
 * no table is compiled into the library; everything is enqueued on `stream`; no host synchronisation, no host read and no
 * allocation inside a call; the number of launches does not depend on B (at most 65535).  A row index is taken from a
 * float32 t the way Colormap.__call__ does: xa = t * 256 (float32); xa < 0 -> row 0, xa >= 256 -> row 255, else trunc(xa).
 * workspace: 4-byte aligned; it is overwritten, its contents on entry do not matter.
 *
 * wmd_viz_disparity (KITTI/test_simple.py:144-175).  disp [B,h,w] float32 -> rgb [B,H,W,3] uint8; optional outputs (NULL to
 * skip): resized [B,H,W] float32, range [B,2] = (vmin, vmax) per image.  Every value of the resized map must be FINITE.
 *   1. resized = wmd_upsample_bilinear_fwd of disp to (H, W) with align_corners = 0 -- that kernel, the same bits; written
 *      once (to `resized`, or to the workspace) and read by every later pass.  (h, w) == (H, W): the map is used as it is.
 *   2. vmin = min of the map.
 *   3. vmax = np.percentile(map, percentile) of a float32 array, whose index arithmetic is float32: n = H W,
 *        qf = (float)percentile / 100.f;  vi = (float)(n - 1) * qf;  k = floor(vi);  g = vi - k;
 *        a = s[k], b = s[min(k + 1, n - 1)] (s = the sorted map);  d = b - a;
 *        vmax = g < 0.5 ? a + d * g : b - d * (1 - g), every operation rounded to float32.
 *      a comes from a three-level radix select (11 + 11 + 10 bits) over the sign-flipped bit patterns, b from the counts of
 *      the last level; nothing is sorted.  -0 and +0 are distinct keys and equal values.
 *   4. vmin == vmax: every pixel gets row 0.  Otherwise Normalize's in-place float32 array with float64 scalars:
 *        t = (float)((double)x - (double)vmin);  t = (float)((double)t / ((double)vmax - (double)vmin));  row as above.
 * Five launches (four when the size does not change).  workspace: wmd_viz_workspace_bytes(B, H, W) bytes (0 for a bad
 * shape; monotone in each argument: 4 (8 + 3 * 2048) bytes of selection state per image, then 4 H W per image for the
 * resized maps); a short one is WMD_ERR_WORKSPACE, tested before its alignment.  Refused before any HIP call: a NULL disp, lut, rgb
 * or workspace, a percentile outside [0, 100] or NaN, a misaligned workspace (WMD_ERR_BAD_ARG); a size < 1
 * (WMD_ERR_BAD_SHAPE); H W >= 2^31 or B > 65535 (WMD_ERR_UNSUPPORTED).
 *
 * wmd_viz_colorize (NYUv2/utils.py:63-82).  x [B,n] float32 -> out uint8 [B,3,n] (channels_first != 0, what the reference
 * returns) or [B,n,3].  All arithmetic float32: t = ((x - vmin) / den), row as above; NaN -> (0, 0, 0), matplotlib's bad
 * colour.  auto_range == 0: vmin and den = (float)(vmax - vmin) come from the caller (den == 0: every pixel row 0);
 * auto_range != 0: vmin = min, den = max - min of every plane on its own (x must be finite; den == 0: row 0), which takes
 * one more launch and a workspace of wmd_viz_workspace_bytes(B, 1, 1) bytes.  Two launches at most.
 *
 * wmd_viz_normalize (KITTI/utils.py:22-28).  x, y [B,n] float32 (finite): y = (x - min) / d in float32, d = (float)((double)max -
 * (double)min), 1e5 when max == min; min and max over every x[b] on its own -- B = 1 with n = the whole tensor is the
 * reference's form.  Two launches; workspace as for the automatic range above.                                          */
size_t wmd_viz_workspace_bytes(int B, int H, int W);
int wmd_viz_disparity(const float* disp, int B, int h, int w, int H, int W, double percentile, const unsigned char* lut,
                      unsigned char* rgb, float* resized, float* range, void* workspace, size_t workspace_bytes, void* stream);
int wmd_viz_colorize(const float* x, int B, size_t n, int auto_range, float vmin, float den, const unsigned char* lut,
                     unsigned char* out, int channels_first, void* workspace, size_t workspace_bytes, void* stream);
int wmd_viz_normalize(const float* x, float* y, int B, size_t n, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ *
 * Pose networks: from the pose trunk's last feature map to cam_T_cam, forward and backward
 * ------------------------------------------------------------------ */

/* transformation_from_parameters (KITTI/layers.py:42-117).  axisangle, translation [N,3], T [N,4,4] row-major.
 *   angle = |v|, a = v / (angle + 1e-7) (not renormalised), R = cos(angle) I + (1 - cos(angle)) a a^T + sin(angle) [a]x
 *   invert == 0: T = [[R, t], [0, 1]]        invert != 0: T = [[R^T, -R^T t], [0, 1]]
 * 1 - cos is evaluated as 2 sin^2(angle / 2).  At v = 0 the rotation block is the identity exactly.
 * Backward: dT [N,4,4] -> d_axisangle, d_translation [N,3], the derivative of the expression above (the 1e-7 included;
 * d|v|/dv = 0 at v = 0, where d_axisangle is exactly 0).  N == 0 is a no-op; one launch each.                          */
int wmd_pose_transform_fwd(const float* axisangle, const float* translation, float* T, int N, int invert, void* stream);
int wmd_pose_transform_bwd(const float* axisangle, const float* translation, const float* dT, float* d_axisangle,
                           float* d_translation, int N, int invert, void* stream);

/* The shared tail of PoseDecoder (pose_decoder.py:43-52) and PoseCNN (pose_cnn.py:42-48): a 1x1 convolution to 6 F
 * channels, the mean over H x W and the 0.01 scale, evaluated with the mean first:
 *   params[b, f, :] = scale * (bias + w . mean_hw(x[b]))      x [B,C,H,W], w [6F,C], bias [6F] or NULL, params [B,F,6]
 * params[b, f, 0:3] is the axis-angle and params[b, f, 3:6] the translation of frame f.  T [B,F,4,4] or NULL: the transform
 * of every frame as above, frame f inverted when bit f of invert_mask is set.  means [B,C] receives mean_hw(x) for the
 * backward.  One launch.  F in 1..4 (WMD_ERR_UNSUPPORTED beyond), (C + 24) floats must fit 64 KB of LDS; H W may be 1
 * and need not be a multiple of 4, C need not be a multiple of 64.                                                       */
int wmd_pose_head_fwd(const float* x, const float* w, const float* bias, float* params, float* T, float* means, int B, int C,
                      int H, int W, int F, int invert_mask, float scale, void* stream);

/* Backward of wmd_pose_head_fwd from d_params [B,F,6] and / or dT [B,F,4,4] (either may be NULL, not both), with the
 * forward's params and means: dx [B,C,H,W], dw [6F,C], dbias [6F] (each may be NULL).  workspace: 6 F B floats.
 * Two launches; the sums over B run in ascending order without atomics, so two runs give the same bits.              */
int wmd_pose_head_bwd(const float* params, const float* means, const float* w, const float* d_params, const float* dT,
                      float* dx, float* dw, float* dbias, float* workspace, int B, int C, int H, int W, int F, int invert_mask,
                      float scale, void* stream);

/* ------------------------------------------------------------------ *
 * Semi-global stereo matching: the candidates of depth-hint fusion
 * ------------------------------------------------------------------ */

/* The matcher of KITTI/precompute_depth_hints.py:42-63,127-151 (StereoSGBM there).  The contract is the integer specification
 * in DESIGN.md ("Semi-global stereo matching"), which follows StereoSGBM's documented parameters and stages; the result
 * equals tests/stereo_ref.py bit for bit and has NOT been compared with OpenCV's.
 *   left, right uint8 [B,H,W,C], C = 1 or 3 (left = the image the map belongs to).  reverse: NULL or B bytes on the device;
 *   image b is mirrored horizontally (both views) before matching and its map mirrored back when reverse[b] != 0.
 *   disp int16 [B,H,W]: 16 x the pixel disparity, (min_disp - 1) * 16 where there is none (always left of column
 *   min_disp + num_disp; right of W - 1 - that with reverse).
 *   cost_out / S_out: NULL or uint16 [B,H,Wv,num_disp], Wv = W - min_disp - num_disp: the block costs and the summed
 *   path costs over the valid rectangle, disparity innermost.
 *   block = blockSize (the window is 2 (block / 2) + 1 wide), cap = preFilterCap, uniq = uniquenessRatio, disp12 =
 *   disp12MaxDiff (<= 0 means 1), directions 5 or 8; speckle_win == 0 skips the speckle stage.
 * workspace: wmd_stereo_sgbm_workspace_bytes(...) bytes, 256-byte aligned, at most about 1 GiB: images that do not fit
 * run in several groups inside the call.  The query returns 0 for arguments the entry refuses.  Per image of a group, each
 * rounded up to 256 bytes and in this order, every region holding the whole group: 16 H W C (prefiltered pairs), 2 H Wv D twice
 * (the two volumes, Wv = W - min_disp - num_disp, D = num_disp), 4 H W (keys), 2 H W (the first map), 8 H W (speckle scratch).
 * Refused before any HIP call: a NULL left / right / disp / workspace, C not 1 or 3, min_disp < 0, num_disp not a multiple
 * of 16 in 16..256, block < 1, P1 < 0 or P1 > P2, directions not 5 or 8, uniq outside 0..100, a negative cap or speckle
 * setting (WMD_ERR_BAD_ARG); a size < 1 or W <= min_disp + num_disp (WMD_ERR_BAD_SHAPE); a short or misaligned workspace
 * (WMD_ERR_WORKSPACE); cap > 127, directions * (win^2 C (2 cap + 63) + P2) > 65535 (S would not fit 16 bits), a window
 * that does not fit the LDS tile, a size above 65535 or more than 2^31 elements (WMD_ERR_UNSUPPORTED).
 * 5 + directions launches and one memset per group, four more with the speckle stage.                                   */
size_t wmd_stereo_sgbm_workspace_bytes(int B, int H, int W, int C, int min_disp, int num_disp, int block);
int wmd_stereo_sgbm(const unsigned char* left, const unsigned char* right, const unsigned char* reverse, short* disp,
                    unsigned short* cost_out, unsigned short* S_out, int B, int H, int W, int C, int min_disp, int num_disp,
                    int block, int P1, int P2, int cap, int uniq, int speckle_win, int speckle_range, int disp12,
                    int directions, void* workspace, size_t workspace_bytes, void* stream);

/* The speckle stage on its own, in place on disp int16 [B,H,W]: every 4-connected component -- neighbours both different
 * from `invalid` and at most max_diff apart; a chain of such steps is one component whatever its ends differ by -- of at
 * most max_size pixels becomes `invalid`.  Union-find over the whole map: a component may cross anything.  workspace:
 * wmd_stereo_filter_speckles_workspace_bytes(B, H, W) bytes = 8 B H W rounded up to 256 (0 for a bad shape), 4-byte aligned;
 * NULL is WMD_ERR_BAD_ARG, short or misaligned WMD_ERR_WORKSPACE.  Four launches.                                         */
size_t wmd_stereo_filter_speckles_workspace_bytes(int B, int H, int W);
int wmd_stereo_filter_speckles(short* disp, int B, int H, int W, int invalid, int max_size, int max_diff, void* workspace,
                               size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WMD_H */
