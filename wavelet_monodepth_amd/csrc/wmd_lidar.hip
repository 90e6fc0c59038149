// KITTI ground-truth depth maps from velodyne scans (KITTI/kitti_utils.py:52-104, generate_depth_map): B scans of a packed
// point list -> [B,H,W] float32, nothing read back to the host.  The reference is a scatter with three ordering rules --
// the last point at a pixel wins, then for every bucket of the linear index sub2ind(v, u) = v (W - 1) + u - 1 that holds
// more than one point the pixel of the bucket's first point receives the bucket's minimum -- and each of them is resolved
// here by an integer atomic on a packed word, so the result does not depend on the order in which points arrive:
//
//   pixel word (64 bit)  = (index + 1) << 32 | value image   atomicMax: the highest index wins and brings its value; 0 = empty
//   key first  (64 bit)  = index << 32 | pixel               atomicMin: the lowest index wins and brings its pixel
//   key min    (32 bit)  = value image                       atomicMin over the bucket
//   key count  (32 bit)                                      atomicAdd; the bucket rule applies from 2
//
// "index" is the point's position in its own scan (< 2^31), "value image" the order-preserving unsigned image of the float32
// value (sign bit flipped for non-negative values, all bits for negative ones): the float64 -> float32 rounding is monotone,
// so the minimum of the rounded values is the rounded minimum.  The bucket index v (W - 1) + u runs over H (W - 1) + 1
// values; with W >= 2 only (v, W - 1) and (v + 1, 0) share one, with W = 1 every pixel does.  The kernels implement the
// bucket rule, not that consequence.
//
// Three launches: lidar_init_kernel fills the workspace (zeros for pixel words and counts, ones for the two minima),
// lidar_scatter_kernel projects every point in float64 without contraction and issues the four atomics of a valid one,
// lidar_resolve_kernel reads a pixel's word and its bucket and writes the float32 map.  Bytes per scan at 375 x 1242
// (465750 pixels, 465377 buckets, N = 120 k): init writes 8 B per pixel + 16 B per bucket = 11.2 MB, the scatter reads
// 16 B per point = 1.9 MB and touches four words per valid point, the resolve reads the 11.2 MB back and writes 1.9 MB.
#include <algorithm>
#include "wmd_internal.h"
#include "wmd_ws_layouts.h"

namespace wmd {

constexpr int kLidarThreads = 256;

// ((P0 x + P1 y) + P2 z) + P3 with every product and sum rounded on its own.  hipcc contracts a * b + c into a fused
// multiply-add by default -- also through __dmul_rn / __dadd_rn, which are plain operators in HIP -- and a fused row moves
// a rounding tie of u or v to the other pixel; the pragma keeps the seven operations apart.
__device__ __forceinline__ double lidar_row(const double* __restrict__ P, double x, double y, double z) {
#pragma clang fp contract(off)
    const double a = P[0] * x, b = P[1] * y, c = P[2] * z;
    const double ab = a + b;
    const double abc = ab + c;
    return abc + P[3];
}

__global__ __launch_bounds__(kLidarThreads) void lidar_init_kernel(unsigned long long* __restrict__ ws, size_t zero_words, size_t total_words) {
    const size_t stride = (size_t)gridDim.x * kLidarThreads;
    for (size_t i = (size_t)blockIdx.x * kLidarThreads + threadIdx.x; i < total_words; i += stride) ws[i] = i < zero_words ? 0ull : ~0ull;
}

// One thread per point of the packed list.  `total` is the host's length of that list: nothing is read beyond it, whatever
// the device-side offsets say, and a point that no scan [offsets[b], offsets[b + 1]) claims is dropped.
__global__ __launch_bounds__(kLidarThreads) void lidar_scatter_kernel(const float4* __restrict__ points, const long long* __restrict__ offsets,
                                                                      const double* __restrict__ P, int B, int H, int W, int vel_depth,
                                                                      long long total, unsigned long long* __restrict__ pix,
                                                                      unsigned* __restrict__ count, unsigned long long* __restrict__ first,
                                                                      unsigned* __restrict__ kmin) {
    const size_t hw = (size_t)H * W, nk = (size_t)H * (W - 1) + 1;
    const long long stride = (long long)gridDim.x * kLidarThreads;
    for (long long i = (long long)blockIdx.x * kLidarThreads + threadIdx.x; i < total; i += stride) {
        const float4 pt = points[i];
        if (!(pt.x >= 0.f)) continue;   // kitti_utils.py:73 -- keeps -0.0, drops NaN; half of a spinning sensor's rows end here
        int lo = 0, hi = B;             // the last b with offsets[b] <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= i) lo = mid; else hi = mid;
        }
        const int b = lo;
        const long long start = offsets[b], idx = i - start;
        if (idx < 0 || i >= offsets[b + 1] || idx >= 0x7fffffffLL) continue;
        const double x = (double)pt.x, y = (double)pt.y, z = (double)pt.z;
        const double* Pb = P + (size_t)b * 12;
        double p[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) p[r] = lidar_row(Pb + r * 4, x, y, z);
        const double u = rint(p[0] / p[2]) - 1.0, v = rint(p[1] / p[2]) - 1.0;
        if (!(u >= 0.0 && v >= 0.0 && u < (double)W && v < (double)H)) continue;   // in float64: inf and NaN drop out here
        const int ui = (int)u, vi = (int)v;
        const unsigned image = order_key((float)(vel_depth ? x : p[2]));
        const size_t pixel = (size_t)vi * W + ui, key = (size_t)vi * (W - 1) + ui;   // sub2ind + 1: 0 .. H (W - 1)
        atomicMax(pix + (size_t)b * hw + pixel, ((unsigned long long)(idx + 1) << 32) | image);
        atomicMin(first + (size_t)b * nk + key, ((unsigned long long)idx << 32) | (unsigned long long)pixel);
        atomicMin(kmin + (size_t)b * nk + key, image);
        atomicAdd(count + (size_t)b * nk + key, 1u);
    }
}

__global__ __launch_bounds__(kLidarThreads) void lidar_resolve_kernel(const unsigned long long* __restrict__ pix, const unsigned* __restrict__ count,
                                                                      const unsigned long long* __restrict__ first,
                                                                      const unsigned* __restrict__ kmin, float* __restrict__ depth, int B, int H,
                                                                      int W) {
    const size_t hw = (size_t)H * W, nk = (size_t)H * (W - 1) + 1, n = (size_t)B * hw;
    const size_t stride = (size_t)gridDim.x * kLidarThreads;
    for (size_t i = (size_t)blockIdx.x * kLidarThreads + threadIdx.x; i < n; i += stride) {
        const size_t b = i / hw;
        const unsigned pixel = (unsigned)(i - b * hw), v = pixel / (unsigned)W, u = pixel - v * (unsigned)W;
        const size_t key = b * nk + (size_t)v * (W - 1) + u;
        const unsigned long long word = pix[i];
        float val = word ? order_unkey((unsigned)word) : 0.f;
        if (count[key] > 1u && (unsigned)first[key] == pixel) val = order_unkey(kmin[key]);   // kitti_utils.py:95-101
        depth[i] = val < 0.f ? 0.f : val;
    }
}

}  // namespace wmd

using namespace wmd;

static bool lidar_shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0; }

extern "C" size_t wmd_lidar_depth_workspace_bytes(int B, int H, int W) {
    if (!lidar_shape_ok(B, H, W) || (double)H * W >= 2147483648.0) return 0;
    return lidar_layout(nullptr, B, H, W).bytes;
}

extern "C" int wmd_lidar_depth_maps(const float* points, const long long* offsets, const double* P, size_t total_points, int B, int H,
                                    int W, int vel_depth, float* depth, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "wmd_lidar_depth_maps";
    if ((!points && total_points != 0) || !offsets || !P || !depth) return fail(WMD_ERR_BAD_ARG, "%s: null tensor pointer", who);
    if (!lidar_shape_ok(B, H, W)) return fail(WMD_ERR_BAD_SHAPE, "%s: B=%d H=%d W=%d must be positive", who, B, H, W);
    if ((size_t)points & 15) return fail(WMD_ERR_BAD_ARG, "%s: points at %p, rows must be 16-byte aligned", who, (const void*)points);
    if ((double)H * W >= 2147483648.0 || total_points >= 2147483648ull)
        return fail(WMD_ERR_UNSUPPORTED, "%s: H*W=%.0f pixels, %zu points: both must stay below 2^31", who, (double)H * W, total_points);
    if (int st = check_workspace(who, workspace, workspace_bytes, lidar_layout(nullptr, B, H, W).bytes, 8, WMD_ERR_WORKSPACE)) return st;
    const LidarWs l = lidar_layout(workspace, B, H, W);
    const size_t total_words = l.bytes / 8;
    hipStream_t s = (hipStream_t)stream;
    const size_t cap = (size_t)kNumCU * 16;   // grid-stride loops: at most 16 blocks of 256 threads per CU
    auto blocks = [cap](size_t n) { return (unsigned)std::min(cap, (n + kLidarThreads - 1) / kLidarThreads); };
    {
        ProfScope prof("lidar_init_kernel", 0.0, 8.0 * total_words, s);
        hipLaunchKernelGGL(lidar_init_kernel, dim3(blocks(total_words)), dim3(kLidarThreads), 0, s, l.pix, l.zero_words, total_words);
    }
    if (total_points > 0) {
        ProfScope prof("lidar_scatter_kernel", 30.0 * (double)total_points, 16.0 * (double)total_points, s);
        // one row per thread (at most 2^23 blocks): the rows are independent and each waits on a chain of dependent loads
        hipLaunchKernelGGL(lidar_scatter_kernel, dim3((unsigned)((total_points + kLidarThreads - 1) / kLidarThreads)), dim3(kLidarThreads), 0, s, (const float4*)points, offsets, P, B, H, W,
                           vel_depth, (long long)total_points, l.pix, l.count, l.first, l.kmin);
    }
    {
        ProfScope prof("lidar_resolve_kernel", 0.0, 8.0 * total_words + 4.0 * B * H * W, s);
        hipLaunchKernelGGL(lidar_resolve_kernel, dim3(blocks((size_t)B * H * W)), dim3(kLidarThreads), 0, s, l.pix, l.count, l.first, l.kmin, depth, B, H,
                           W);
    }
    return check_launch("lidar kernels");
}
