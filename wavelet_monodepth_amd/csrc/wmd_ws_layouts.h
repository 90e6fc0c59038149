// The workspace layouts of the data, loss and evaluation operators, each written once: a layout function takes its regions from a
// WsLayout (wmd_internal.h) in the order they lie in memory -- a braced list is evaluated left to right -- and returns them as typed
// pointers, with the bytes.  The entry's size query calls it with a null workspace, its launch with the caller's pointer, after
// check_workspace.  Host code only, no HIP call: tests/ws_layout_host.cpp walks every function here.
#pragma once
#include "wmd_select.h"   // SEL_STATE: a radix selection's state, uint32 per image

namespace wmd {

constexpr int DBE_STATE = 208;   // the depth-boundary state, uint32 per image: min key, max key, n_est, n_gt, histA[101], histB[101]

// wmd_eval_kitti, in a float workspace.  The prefix -- two [B,plane] planes, [B] counts, [B,2] medians -- is what include/wmd.h promises at
// wmd_eval_workspace_floats: evaluation.kitti_metrics reads the medians back at float 2 * B * plane + B.  Behind it two selection states
// per image and the [B,64,9] fp64 partial error sums.
struct EvalWs { float *pred, *gt; int* count; float* med; unsigned* state; double* partial; size_t bytes; };
inline EvalWs eval_layout(float* ws, size_t B, size_t plane) {
    WsLayout l(ws, alignof(float));
    return {l.take<float>(B * plane), l.take<float>(B * plane), l.take<int>(B), l.take<float>(B * 2), l.take<unsigned>(B * 2 * SEL_STATE),
            l.take<double>(B * 64 * 9), l.bytes()};
}

// wmd_eval_canny / wmd_eval_dbe: the normalisation and chamfer state, the smoothed image in fp64, three bit planes of Wp words a row
struct DbeWs { unsigned* state; double* sm; unsigned *weak, *strong, *gt; size_t bytes; };
inline DbeWs dbe_layout(void* ws, size_t B, size_t H, size_t W, size_t Wp) {
    WsLayout l(ws, 8);
    return {l.take<unsigned>(B * DBE_STATE), l.take<double>(B * H * W), l.take<unsigned>(B * H * Wp), l.take<unsigned>(B * H * Wp),
            l.take<unsigned>(B * H * Wp), l.bytes()};
}

// wmd_viz_*: the selection state of every image, then one resized plane per image (plane = 0: normalize and colorize need the state alone)
struct VizWs { unsigned* state; float* resized; size_t bytes; };
inline VizWs viz_layout(void* ws, size_t B, size_t plane) {
    WsLayout l(ws, 4);
    return {l.take<unsigned>(B * SEL_STATE), l.take<float>(B * plane), l.bytes()};
}

// wmd_lidar_depth_maps: hw pixel words and nk bucket counts per scan, which lidar_init_kernel zeroes, then the buckets' first words and
// minima, which it fills with ones; every array padded to 8 bytes.  zero_words: where the ones begin, in 64-bit words.
struct LidarWs { unsigned long long* pix; unsigned* count; unsigned long long* first; size_t zero_words; unsigned* kmin; size_t bytes; };
inline LidarWs lidar_layout(void* ws, size_t B, size_t H, size_t W) {
    const size_t hw = H * W, nk = H * (W - 1) + 1;
    WsLayout l(ws, 8);
    return {l.take<unsigned long long>(B * hw), l.take<unsigned>(B * nk), l.take<unsigned long long>(B * nk), l.bytes() / 8 - B * nk,
            l.take<unsigned>(B * nk), (l.take<char>(0, 8), l.bytes())};
}

// one region of n elements: the 64-bit grey sums of wmd_color_pyramid (levels x images) and wmd_color_jitter (images); the floats of
// wmd_ssim_bwd (three coefficient planes per element) and wmd_warp_bwd (12 partial sums per block and image); and, in a float workspace,
// the fp64 partial sums of wmd_smooth_fwd (two per block)
template <class T> struct ArrayWs { T* p; size_t bytes; };
template <class T> inline ArrayWs<T> array_layout(void* ws, size_t n, size_t base_align = alignof(T)) {
    WsLayout l(ws, base_align);
    return {l.take<T>(n), l.bytes()};
}

// wmd_stereo_filter_speckles (a 4-byte aligned workspace), and the last region of wmd_stereo_sgbm: a label and a count per pixel; the
// total padded to 256 bytes, which is what the regions of the matcher's workspace are sized in
struct SpeckleWs { int *labels, *counts; size_t bytes; };
inline SpeckleWs speckle_layout(void* ws, size_t n) {
    WsLayout l(ws, 4);
    return {l.take<int>(n), l.take<int>(n), (l.take<char>(0, 256), l.bytes())};
}

// wmd_stereo_sgbm, for a group of images: [group][2][H][W][C] prefiltered pairs, the two volumes, [group][H][W] keys and first maps, speckle
// scratch.  Every image of a region is padded to a multiple of 256 bytes: it starts stereo_stride<T>(n) elements after the one before it.
template <class T> inline size_t stereo_stride(size_t n) { return (n * sizeof(T) + 255) / 256 * 256 / sizeof(T); }
struct StereoWs { uint2* prep; uint16_t *cost, *S; unsigned* keys; int16_t* first_map; void* speckle; size_t bytes; };
inline StereoWs stereo_layout(void* ws, size_t group, size_t H, size_t W, size_t C, size_t volume) {
    WsLayout l(ws, 256);
    const size_t vol = group * stereo_stride<uint16_t>(volume);
    return {l.take<uint2>(group * stereo_stride<uint2>(2 * H * W * C), 256), l.take<uint16_t>(vol, 256), l.take<uint16_t>(vol, 256),
            l.take<unsigned>(group * stereo_stride<unsigned>(H * W), 256), l.take<int16_t>(group * stereo_stride<int16_t>(H * W), 256),
            l.take<char>(group * speckle_layout(nullptr, H * W).bytes, 256), l.bytes()};
}

}  // namespace wmd
