// Internal helpers shared by the HIP translation units of libwmd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>
#include <utility>
#include "../../include/wmd.h"

namespace wmd {

void set_error(const char* fmt, ...);

inline int fail(int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    set_error("%s", buf);
    return status;
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WMD_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return WMD_OK;
}

// A caller's workspace, described once per entry (wmd_ws_layouts.h): a layout function takes the regions in order; the size query runs it on
// a null base, the launch on the caller's pointer, of which the entry's check guarantees `base_align`.  A region aligned beyond that (fp64
// partials in a float workspace) gets `align` spare bytes and its real address rounded up.  take<char>(0, a) only pads the offset to a.
struct WsLayout {
    char* base;
    size_t base_align, off = 0;
    WsLayout(void* ws, size_t guaranteed_align) : base(static_cast<char*>(ws)), base_align(guaranteed_align) {}
    template <class T>
    T* take(size_t count, size_t align = alignof(T)) {
        const bool spare = count && align > base_align;   // otherwise offsets round relative to the base
        const uintptr_t real = spare ? reinterpret_cast<uintptr_t>(base) : 0;
        const size_t at = (real + off + align - 1) / align * align - real;
        off = (spare ? off + align : at) + count * sizeof(T);
        return base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
    size_t bytes() const { return off; }
};

// The one workspace refusal: NULL, then short (both WMD_ERR_WORKSPACE), then misaligned -- with the entry's documented answer (include/wmd.h:
// WMD_ERR_BAD_ARG for the colour images and the depth-boundary errors, WMD_ERR_WORKSPACE elsewhere).  An entry that answers a NULL workspace
// with WMD_ERR_BAD_ARG refuses it with its other pointers, before this.  NULL passes only where nothing is needed and nothing is claimed.
inline int check_workspace(const char* who, const void* ws, size_t have, size_t need, size_t align, int misaligned_status) {
    const bool null = !ws && (have || need), misaligned = reinterpret_cast<uintptr_t>(ws) % align != 0;
    if (!null && have >= need && !misaligned) return WMD_OK;
    return fail(null || have < need ? WMD_ERR_WORKSPACE : misaligned_status, "%s: workspace %zu bytes at %p, %zu needed, %zu-byte aligned", who, have, ws,
                need, align);
}
// the entries that count floats: no alignment is asked of a float pointer
inline int check_workspace_floats(const char* who, const float* ws, size_t have, size_t need) {
    const size_t cap = ~(size_t)0 / sizeof(float);
    return check_workspace(who, ws, (have < cap ? have : cap) * sizeof(float), need * sizeof(float), 1, WMD_ERR_WORKSPACE);
}

constexpr int kNumCU = 256;  // MI355X

// Opt-in per-launch timing (wmd_profile_begin/end). Zero cost when off: one predictable branch.
extern bool g_prof_on;
int prof_open(const char* name, double flops, double bytes, hipStream_t s);
void prof_close(int idx, hipStream_t s);
void prof_set_mfma(int idx, double mfma_flops);   // FLOPs the matrix pipe executes for this launch (default: the algorithmic count)
struct ProfScope {
    int idx;
    hipStream_t s;
    ProfScope(const char* name, double flops, double bytes, hipStream_t stream) : idx(-1), s(stream) {
        if (g_prof_on) idx = prof_open(name, flops, bytes, stream);
    }
    void mfma(double f) {
        if (idx >= 0) prof_set_mfma(idx, f);
    }
    ~ProfScope() {
        if (idx >= 0) prof_close(idx, s);
    }
};

__device__ __forceinline__ float act_apply(float v, int act, float slope) {
    switch (act) {
        case WMD_ACT_ELU: return v > 0.f ? v : expm1f(v);
        case WMD_ACT_LEAKY: return v > 0.f ? v : v * slope;
        case WMD_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        default: return v;
    }
}

// f'(x) written in terms of the activation OUTPUT y = f(x)
__device__ __forceinline__ float act_deriv(float y, int act, float slope) {
    switch (act) {
        case WMD_ACT_ELU: return y > 0.f ? 1.f : y + 1.f;     // y = e^x - 1  =>  dy/dx = y + 1
        case WMD_ACT_LEAKY: return y > 0.f ? 1.f : slope;
        case WMD_ACT_SIGMOID: return y * (1.f - y);
        default: return 1.f;
    }
}

// map a padded coordinate g in [-1, n] to a source coordinate; returns false when the tap reads zero
__device__ __forceinline__ bool pad_coord(int& g, int n, int pad_mode) {
    if (pad_mode == WMD_PAD_REFLECT) {
        if (g < 0) g = -g;
        if (g >= n) g = 2 * n - 2 - g;
    } else if (pad_mode == WMD_PAD_REPLICATE) {
        g = g < 0 ? 0 : (g >= n ? n - 1 : g);
    } else {
        if (g < 0 || g >= n) return false;
    }
    return true;
}

// The same map branch-free, for code every block of a launch runs at the same moment (the 32x32x2 Winograd kernels' offset
// prologues: nothing hides them, and pad_coord's switch per coordinate with short-circuit tests cost 16 k cycles per block on
// L14, cycle stamps): the pad mode is uniform, everything is a select.  Returns the source coordinate of padded coordinate g in
// [-1, n] and clears `ok` on a zero-pad miss; a coordinate beyond the ring (tile overhang) gives some in-range pixel that is
// never stored.
__host__ __device__ __forceinline__ int pad_fold(int pad_mode, int g, int n, int& ok) {
    const int refl = g < 0 ? -g : (g >= n ? 2 * n - 2 - g : g);
    const int clam = min(max(g, 0), n - 1);
    ok &= (int)(pad_mode != WMD_PAD_ZERO) | (int)(g == clam);
    const int r = pad_mode == WMD_PAD_REFLECT ? refl : clam;
    return min(max(r, 0), n - 1);
}

// compile-time loop: f(integral_constant<int, I>) for I = 0 .. N-1, expanded by the front end (a `#pragma unroll` loop over
// the MFMA groups with the piece test inside exceeds the optimizer's full-unroll budget, and a rolled loop would index the
// accumulators at run time)
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Order-preserving float <-> uint32 key: unsigned order of the keys is float order of the values, with -0 < +0 (and NaNs
// beyond the infinity of their sign); the inverse is exact, order_unkey(order_key(f)) has f's bits.
__device__ __forceinline__ unsigned order_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// wmd_conv_fwd.hip: the fused convolution's contract (include/wmd.h, at wmd_conv_args), under the entry point's name `who`.  Every entry
// that takes the problem calls conv_check_problem before its own rules (act: WMD_ACT_NONE where the entry has no activation); it reads no
// pointer, so the shape queries answer from it alone.  conv_check_tensors: x1 / wp / y, and x2 when C2 > 0 -- the entries that launch.
int conv_check_problem(int B, int H, int W, int C1, int up1, int C2, int Cout, int ksize, int pad_mode, int act, const char* who);
int conv_check_tensors(const wmd_conv_args* g, const char* who);

// The wavelet heads' front end.  Every WMD_HEAD* / WMD_SHIFTSUM* switch, read once per process (wmd_head.hip):
struct HeadSwitches {
    bool chain;              // WMD_HEAD_CHAIN=0: the two-launch heads stay on the FUSE form of conv_fwd_kernel
    bool chain_multi;        // WMD_HEAD_CHAIN_MULTI=0 (or chain off): every level's first stage as a launch of its own
    int chain_pg256;         // WMD_HEAD_CHAIN_PG256=2 / 3 forces the C = 256 chain block to 32 / 48 pixels (0: by block count)
    bool stream;             // WMD_HEAD_STREAM=0: the C = 32 level stays on head_level_kernel
    int stream_th;           // WMD_HEAD_STREAM_TH=<rows> forces the streaming kernel's segment height (0: the host's model)
    long stream_min_pixels;  // WMD_HEAD_STREAM_MIN_PIXELS: B*H*W from which the streaming kernel runs (0)
    bool shiftsum_square;    // WMD_SHIFTSUM_CHAIN_SQUARE=1: 4 x 4 completion tiles instead of 2 x 8
    int csplit;              // WMD_HEAD_CSPLIT=<n> forces head3x3_kernel's channel split (0: the planner's)
    int ng;                  // WMD_HEAD_NG=<n> forces head3x3_kernel's channel groups: 4, anything else 2 (0: by tile count)
    bool bwd_fused;          // WMD_HEAD_BWD_FUSED=0: the C = 32 backward never runs as head_bwd_fused32_kernel
};
const HeadSwitches& head_switches();
// what ProfScope records for the two GEMMs of a level's +- heads, and for the bytes of a level that ends in yh (+ out (+ disp))
inline double head_gemm_flops(double pix, int C) { return 2.0 * pix * (2.0 * C * C + 54.0 * C); }
inline double head_level_bytes(double pix, int in_planes, bool out, bool disp) { return 4.0 * pix * (in_planes + 3 + (out ? (disp ? 9 : 5) : 0)); }
// wmd_head.hip, under the entry point's name `fn`: the pad mode's range and H, W >= 2 for reflect; the per-level rules of a completion
// chain (level k, coarse to fine, must be B x H x W), for wmd_head_shiftsum_chain_fwd and -- `coarse` -- wmd_head_level_pyramid_fwd
int head_check_pad(const char* fn, int pad_mode, int H, int W);
int head_check_completion_level(const char* fn, bool coarse, int k, const wmd_head_shiftsum_args& c, int B, int H, int W);
// wmd_conv_fwd.hip: the FUSE instantiations of conv_fwd_kernel, for what the chained kernel of wmd_head_chain.hip does not take -- a level's +- heads
// (wp1 / bias1 / wp2 = both sides stacked) or, low_pass, the low-pass chain alone (C = 256 -> planes 54..62 of an 81-plane t)
int head_fuse_launch(const float* x, const float* wp1, const float* bias1, const float* wp2, float* t, int B, int plane, int C, float slope, int t_planes, bool low_pass, hipStream_t s);

// wmd_head_stream.hip: the streaming form of wmd_head_level_fwd (C = 32, plain inference outputs); 0 = not taken
int head_stream_launch(const wmd_head_level_args* g, const wmd_head_shiftsum_args* coarse, int n_coarse, hipStream_t s);
int head_stream_pyramid_pays(int B, int H, int W);

}  // namespace wmd
