// Host walk of the workspace layouts of the data, loss and evaluation operators (wmd_ws_layouts.h), built and run by
// test_ws_layout_host.py, once plain and once under the address and undefined-behaviour sanitizers.  Calls no HIP API.
//
// For every layout function and shape: sizing on a null workspace gives the bytes that carving a real buffer gives; every region
// lies inside those bytes, starts at its type's alignment, and no two overlap; and every region starts where include/wmd.h says
// it does -- the closed forms are written out here from its comments, not taken from the code under test.  The layouts that put
// fp64 partials into a float workspace are carved a second time at a base that is 4 mod 8.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../wavelet_monodepth_amd/csrc/wmd_ws_layouts.h"

using namespace wmd;

static long g_checked = 0, g_failed = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        ++g_checked;                                       \
        if (!(cond)) {                                     \
            if (++g_failed <= 20) {                        \
                std::printf("FAIL %s: ", #cond);           \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
        }                                                  \
    } while (0)

struct Region {
    const char* name;
    const void* p;
    size_t bytes, align, want;   // want: the byte offset the documentation gives (kRounded: the first aligned address at or after `from`)
    size_t from;
};
constexpr size_t kRounded = ~(size_t)0;

// a buffer of `bytes` (at least one) whose start is `rem` modulo 256
struct Buffer {
    char* raw;
    char* base;
    Buffer(size_t bytes, size_t rem) : raw((char*)std::malloc(bytes + 512)) {
        base = (char*)(((uintptr_t)raw + 255) / 256 * 256 + rem);
        std::memset(base, 0xA5, bytes);   // the sanitizer sees every byte the layout claims
    }
    ~Buffer() { std::free(raw); }
};

static void check_regions(const char* what, const char* base, size_t sized, size_t carved, const std::vector<Region>& rs) {
    CHECK(sized == carved, "%s: sized %zu, carved %zu", what, sized, carved);
    for (size_t i = 0; i < rs.size(); ++i) {
        const Region& r = rs[i];
        const char* p = (const char*)r.p;
        CHECK(p >= base && p + r.bytes <= base + sized, "%s.%s: [%td, %td) outside %zu bytes", what, r.name, p - base, p - base + (ptrdiff_t)r.bytes, sized);
        CHECK((uintptr_t)p % r.align == 0, "%s.%s: %p not %zu-byte aligned", what, r.name, r.p, r.align);
        const size_t want = r.want != kRounded ? r.want : (size_t)(((uintptr_t)base + r.from + r.align - 1) / r.align * r.align - (uintptr_t)base);
        CHECK((size_t)(p - base) == want, "%s.%s: offset %td, %zu documented", what, r.name, p - base, want);
        for (size_t j = 0; j < i; ++j) {
            const char* q = (const char*)rs[j].p;
            CHECK(p + r.bytes <= q || q + rs[j].bytes <= p || !r.bytes || !rs[j].bytes, "%s: %s and %s overlap", what, r.name, rs[j].name);
        }
    }
}

static const size_t SEL = 4 * (8 + 3 * 2048);   // bytes of a selection state (include/wmd.h, at wmd_viz_disparity)

static void eval_case(size_t B, size_t H, size_t W, size_t rem) {
    const size_t sized = eval_layout(nullptr, B, H * W).bytes, P = 4 * B * H * W;
    Buffer buf(sized, rem);
    const EvalWs w = eval_layout((float*)buf.base, B, H * W);
    const size_t carved = w.bytes;
    // include/wmd.h at wmd_eval_workspace_floats: two [B,H,W] planes, [B] counts, [B,2] medians; then the library's own
    const size_t tail = 2 * P + 12 * B + 2 * B * SEL;
    check_regions("eval", buf.base, sized, carved,
                  {{"pred", w.pred, P, 4, 0, 0}, {"gt", w.gt, P, 4, P, 0}, {"count", w.count, 4 * B, 4, 2 * P, 0}, {"med", w.med, 8 * B, 4, 2 * P + 4 * B, 0},
                   {"state", w.state, 2 * B * SEL, 4, 2 * P + 12 * B, 0}, {"partial", w.partial, 8 * B * 64 * 9, 8, kRounded, tail}});
    CHECK(sized == tail + 8 * B * 64 * 9 + 8, "eval: %zu bytes", sized);   // two floats of slack
}

static void smooth_case(size_t nblk, size_t rem) {
    const size_t sized = array_layout<double>(nullptr, 2 * nblk, alignof(float)).bytes;   // as wmd_smooth_fwd calls it
    Buffer buf(sized, rem);
    const ArrayWs<double> w = array_layout<double>(buf.base, 2 * nblk, alignof(float));
    const size_t carved = w.bytes;
    check_regions("smooth", buf.base, sized, carved, {{"partial", w.p, 16 * nblk, 8, kRounded, 0}});
    CHECK(sized == 16 * nblk + 8, "smooth: %zu bytes", sized);
}

static void dbe_case(size_t B, size_t H, size_t W) {
    const size_t Wp = 2 * ((W + 63) / 64), sized = dbe_layout(nullptr, B, H, W, Wp).bytes;
    Buffer buf(sized, 8);
    const DbeWs w = dbe_layout(buf.base, B, H, W, Wp);
    const size_t carved = w.bytes;
    const size_t st = 832 * B, sm = 8 * B * H * W, pl = 4 * B * H * Wp;   // include/wmd.h at wmd_eval_dbe_workspace_bytes
    check_regions("dbe", buf.base, sized, carved,
                  {{"state", w.state, st, 4, 0, 0}, {"sm", w.sm, sm, 8, st, 0}, {"weak", w.weak, pl, 4, st + sm, 0},
                   {"strong", w.strong, pl, 4, st + sm + pl, 0}, {"gt", w.gt, pl, 4, st + sm + 2 * pl, 0}});
    CHECK(sized == st + sm + 3 * pl, "dbe: %zu bytes", sized);
}

static void viz_case(size_t B, size_t plane) {
    const size_t sized = viz_layout(nullptr, B, plane).bytes;
    Buffer buf(sized, 4);
    const VizWs w = viz_layout(buf.base, B, plane);
    const size_t carved = w.bytes;
    check_regions("viz", buf.base, sized, carved, {{"state", w.state, B * SEL, 4, 0, 0}, {"resized", w.resized, 4 * B * plane, 4, B * SEL, 0}});
    CHECK(sized == B * SEL + 4 * B * plane, "viz: %zu bytes", sized);
}

static void lidar_case(size_t B, size_t H, size_t W) {
    const LidarWs n = lidar_layout(nullptr, B, H, W);
    const size_t sized = n.bytes;
    Buffer buf(sized, 8);
    const LidarWs w = lidar_layout(buf.base, B, H, W);
    const size_t carved = w.bytes;
    // 8 bytes per pixel word, 8 + 4 + 4 per bucket of sub2ind (H (W - 1) + 1 of them), each array padded to 8 bytes
    const size_t nk = B * (H * (W - 1) + 1), pix = 8 * B * H * W, half = 8 * ((nk + 1) / 2);
    check_regions("lidar", buf.base, sized, carved,
                  {{"pix", w.pix, pix, 8, 0, 0}, {"count", w.count, 4 * nk, 4, pix, 0}, {"first", w.first, 8 * nk, 8, pix + half, 0},
                   {"kmin", w.kmin, 4 * nk, 4, pix + half + 8 * nk, 0}});
    CHECK(sized == pix + 8 * nk + 2 * half, "lidar: %zu bytes", sized);
    CHECK(w.zero_words == (pix + half) / 8 && n.zero_words == w.zero_words, "lidar: zero_words %zu sized, %zu carved", n.zero_words, w.zero_words);
}

static void sums_case(size_t count) {
    const size_t sized = array_layout<unsigned long long>(nullptr, count).bytes;
    Buffer buf(sized, 8);
    const ArrayWs<unsigned long long> w = array_layout<unsigned long long>(buf.base, count);
    const size_t carved = w.bytes;
    check_regions("grey sums", buf.base, sized, carved, {{"sums", w.p, 8 * count, 8, 0, 0}});
    CHECK(sized == 8 * count, "grey sums: %zu bytes", sized);
}

static size_t up256(size_t n) { return (n + 255) / 256 * 256; }

static void speckle_case(size_t px) {
    const size_t sized = speckle_layout(nullptr, px).bytes;
    Buffer buf(sized, 4);
    const SpeckleWs w = speckle_layout(buf.base, px);
    const size_t carved = w.bytes;
    check_regions("speckle", buf.base, sized, carved, {{"labels", w.labels, 4 * px, 4, 0, 0}, {"counts", w.counts, 4 * px, 4, 4 * px, 0}});
    CHECK(sized == up256(8 * px), "speckle: %zu bytes", sized);
}

static void stereo_case(size_t G, size_t H, size_t W, size_t C, size_t min_disp, size_t D) {
    const size_t vol = H * (W - min_disp - D) * D, sized = stereo_layout(nullptr, G, H, W, C, vol).bytes;
    Buffer buf(sized, 0);
    const StereoWs w = stereo_layout(buf.base, G, H, W, C, vol);
    const size_t carved = w.bytes;
    // include/wmd.h at wmd_stereo_sgbm: per image, each rounded up to 256 bytes, every region holding the whole group
    const size_t prep = G * up256(16 * H * W * C), v = G * up256(2 * vol), keys = G * up256(4 * H * W), map = G * up256(2 * H * W), sp = G * up256(8 * H * W);
    check_regions("stereo", buf.base, sized, carved,
                  {{"prep", w.prep, prep, 256, 0, 0}, {"cost", w.cost, v, 256, prep, 0}, {"S", w.S, v, 256, prep + v, 0},
                   {"keys", w.keys, keys, 256, prep + 2 * v, 0}, {"first_map", w.first_map, map, 256, prep + 2 * v + keys, 0},
                   {"speckle", w.speckle, sp, 256, prep + 2 * v + keys + map, 0}});
    CHECK(sized == prep + 2 * v + keys + map + sp, "stereo: %zu bytes", sized);
    CHECK(stereo_stride<uint16_t>(vol) * 2 == up256(2 * vol), "stereo: volume stride %zu", stereo_stride<uint16_t>(vol));
    CHECK(speckle_layout(w.speckle, G * H * W).bytes <= sp, "stereo: the group's speckle scratch exceeds its region");
}

static void floats_case(size_t B, size_t C, size_t H, size_t W, size_t nblk) {
    for (size_t floats : {3 * B * C * H * W, 12 * B * nblk}) {   // wmd_ssim_bwd: 3 B C H W floats; wmd_warp_bwd: 12 per block and image
        const size_t sized = array_layout<float>(nullptr, floats).bytes;
        Buffer buf(sized, 4);
        const ArrayWs<float> w = array_layout<float>(buf.base, floats);
        check_regions("floats", buf.base, sized, w.bytes, {{"floats", w.p, 4 * floats, 4, 0, 0}});
        CHECK(sized == 4 * floats, "floats: %zu bytes", sized);
    }
}

int main() {
    const size_t eval_shapes[][3] = {{2, 11, 37}, {2, 96, 128}, {1, 375, 1242}, {16, 375, 1242}, {1, 1, 1}};
    for (auto& s : eval_shapes)
        for (size_t rem : {0, 4, 8, 12}) eval_case(s[0], s[1], s[2], rem);
    for (size_t nblk : {1, 2, 512, 60, 3})
        for (size_t rem : {0, 4, 8, 12}) smooth_case(nblk, rem);
    const size_t dbe_shapes[][3] = {{2, 48, 64}, {1, 23, 70}, {2, 23, 70}, {1, 3, 3}, {4, 480, 640}};
    for (auto& s : dbe_shapes) dbe_case(s[0], s[1], s[2]);
    const size_t viz_shapes[][2] = {{2, 11 * 37}, {1, 1}, {13, 375 * 1242}, {2, 0}, {3, 5}};
    for (auto& s : viz_shapes) viz_case(s[0], s[1]);
    const size_t lidar_shapes[][3] = {{1, 6, 8}, {5, 8, 12}, {2, 5, 1}, {3, 4, 2}, {64, 375, 1242}};
    for (auto& s : lidar_shapes) lidar_case(s[0], s[1], s[2]);
    for (size_t n : {3, 26, 12, 1, 65535, 4 * 12, 8 * 65535}) sums_case(n);
    for (size_t px : {2 * 9 * 11, 3 * 12 * 48, 375 * 1242, 1, 4 * 32 * 32}) speckle_case(px);
    const size_t stereo_shapes[][6] = {{3, 12, 48, 1, 0, 16}, {3, 12, 48, 3, 0, 16}, {1, 375, 1242, 3, 0, 96}, {4, 96, 320, 3, 0, 96}, {2, 37, 211, 3, 5, 160}};
    for (auto& s : stereo_shapes) stereo_case(s[0], s[1], s[2], s[3], s[4], s[5]);
    const size_t float_shapes[][5] = {{1, 3, 4, 5, 1}, {2, 3, 40, 32, 2}, {12, 3, 192, 640, 120}, {1, 1, 2, 2, 1}, {2, 3, 6, 8, 1}};
    for (auto& s : float_shapes) floats_case(s[0], s[1], s[2], s[3], s[4]);
    std::printf("%ld checks, %ld failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
