// Host walk of the gather-offset arithmetic of the 32x32x2 Winograd kernels' staging front end (wmd_conv_wino32_stage.h), built and
// run by test_wino32_stage_host.py.  Calls no HIP API.
//
// Two routes to the byte offset a patch position is staged from:
//   table:  w32_tab_entry (w32_full_rc / w32_low_rc per patch row and column) + w32_off_full / w32_off_low = channel * plane + row + column
//   rule:   per position, as conv_wino32_kernel's GENERIC staging states it (full_pos): fold each padded coordinate; a zero-pad miss or
//           a coordinate beyond the pad ring reads nothing; then >> 1 for an upsampled operand, else - shift1 with the bounds test
//           against H1 x W1.  Restated here with pad_coord's case analysis, not through pad_fold.
// For every patch position of every 2x2 Winograd tile with an output pixel inside the image both must read zero or give the same
// offset; on the upsampled operand the low-resolution cell compared is the one the UP transform reads for patch position (r, c) of
// tile (tyy, txx): row tyy + (r + 1) / 2, column txx + (c + 1) / 2.  The 16-byte form: w32_x4_ok holds exactly when the whole patch
// row lies inside the source row, and then every piece's offset + 4 k is the dword offset of its k-th column.  The same-size and the
// upsampled maps are walked a second time through the in-mask forms: a position whose folded pixel is masked out reads zero.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../wavelet_monodepth_amd/csrc/wmd_conv_wino32_stage.h"

using namespace wmd;

static long g_checked = 0, g_failed = 0, g_x4_tiles = 0, g_low = 0;

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

// the rule, one coordinate: false = reads nothing
static bool rule_coord(int g0, int n, int pad_mode, int& g) {
    if (g0 > n) return false;   // beyond the pad ring (tile overhang)
    g = g0;
    if (pad_mode == WMD_PAD_REFLECT) {
        if (g < 0) g = -g;
        if (g >= n) g = 2 * n - 2 - g;
    } else if (pad_mode == WMD_PAD_REPLICATE) {
        g = g < 0 ? 0 : (g >= n ? n - 1 : g);
    } else if (g < 0 || g >= n) {
        return false;
    }
    return true;
}
// the rule, one position of x2's geometry (H x W) / of x1's (H1 x W1 through up1 / shift1): kOOB or the byte offset inside a plane
static void rule_pos(const ConvKArgs& a, int gy0, int gx0, unsigned& o1, unsigned& o2, int& gy, int& gx) {
    gy = gx = 0;
    const bool ok = rule_coord(gy0, a.H, a.pad_mode, gy) && rule_coord(gx0, a.W, a.pad_mode, gx);
    o2 = ok ? (unsigned)(gy * a.W + gx) * 4u : kOOB;
    const int sy = a.up1 == 2 ? gy >> 1 : gy - a.shift1, sx = a.up1 == 2 ? gx >> 1 : gx - a.shift1;
    const bool ok1 = ok && sy >= 0 && sx >= 0 && sy < a.H1 && sx < a.W1;
    o1 = ok1 ? (unsigned)(sy * a.W1 + sx) * 4u : kOOB;
}

// masked: the in-mask forms (MASKED = true) under a mask plane that is constant on aligned 2x2 blocks (what wino32_pure asks of an
// upsampled launch), about a third of it zero; the mask lives on the H x W geometry, so not on a data-gradient launch
template <class T, int CK>
static void walk_map(ConvKArgs a, bool masked) {
    constexpr int TH = T::TILE_H, TW = T::TILE_W, PH = T::PH, PWS = T::PWS, PSF = T::PSF, PHL = T::PHL, PWL = T::PWL, PSL = T::PSL;
    const bool up = a.up1 == 2;
    const W32Planes pl = w32_planes(a);
    const unsigned pbs = up ? pl.pb2 : pl.pb1;
    const int chans[3] = {0, 1, CK - 1};
    std::vector<int> tab(T::TAB_FLOATS);
    std::vector<uint8_t> mask((size_t)a.H * a.W);
    for (int y = 0; y < a.H; ++y)
        for (int x = 0; x < a.W; ++x) mask[(size_t)y * a.W + x] = (((y >> 1) * 7 + (x >> 1) * 13 + a.H) % 3) != 0;
    if (masked) a.in_mask = mask.data(), a.in_mask_2x2 = 1;
    a.tiles_y = (a.H + TH - 1) / TH, a.tiles_x = (a.W + TW - 1) / TW;
    for (int ty = 0; ty < a.tiles_y; ++ty)
        for (int tx = 0; tx < a.tiles_x; ++tx) {
            const int y0 = ty * TH, x0 = tx * TW;
            std::fill(tab.begin(), tab.end(), 0x7fffffff);
            for (int t = 0; t < T::TAB_FLOATS + 8; ++t) w32_tab_entry<T>(a, y0, x0, tab.data(), t);   // threads beyond the table write nothing
            for (int t = PH + PWS + PHL + PWL; t < T::TAB_FLOATS; ++t) CHECK(tab[t] == 0x7fffffff, "table entry %d written", t);
            // ---- dword pieces against the rule ------------------------------------------------------------------------
            for (int tyy = 0; tyy < T::TYB; ++tyy)
                for (int txx = 0; txx < T::TXB; ++txx) {
                    if (y0 + 2 * tyy >= a.H || x0 + 2 * txx >= a.W) continue;   // no output pixel inside the image
                    for (int r = 0; r < 4; ++r)
                        for (int c = 0; c < 4; ++c) {
                            const int py = 2 * tyy + r, px = 2 * txx + c;
                            unsigned o1, o2;
                            int gy, gx;
                            rule_pos(a, y0 + py - 1, x0 + px - 1, o1, o2, gy, gx);
                            const bool live = !masked || mask[(size_t)gy * a.W + gx] != 0;   // the mask test follows the coordinate padding
                            const unsigned want_in = up ? o2 : o1;   // the full-resolution run: the skip tensor beside an upsampled x1, else x1
                            for (int ch : chans) {
                                const unsigned e = (unsigned)(ch * PSF + py * PWS + px);
                                const unsigned got = masked ? w32_off_full<T, CK, true>(a, pl, tab.data(), mask.data(), e)
                                                            : w32_off_full<T, CK, false>(a, pl, tab.data(), nullptr, e);
                                const unsigned want = want_in == kOOB || !live ? kOOB : ch * pbs + want_in;
                                CHECK(got == want, "full %dx%d H=%d W=%d pad=%d up=%d shift=%d tile (%d,%d) pos (%d,%d) ch %d: table %u, rule %u", TH,
                                      TW, a.H, a.W, a.pad_mode, a.up1, a.shift1, ty, tx, py, px, ch, got, want);
                                if (!up) continue;
                                ++g_low;
                                const int ly = tyy + (r + 1) / 2, lx = txx + (c + 1) / 2;   // the cell the UP transform reads
                                const unsigned el = (unsigned)(ch * PSL + ly * PWL + lx);
                                const unsigned gotl = masked ? w32_off_low<T, CK, true>(a, pl, tab.data(), mask.data(), el)
                                                             : w32_off_low<T, CK, false>(a, pl, tab.data(), nullptr, el);
                                const unsigned wantl = o1 == kOOB || !live ? kOOB : ch * pl.pb1 + o1;
                                CHECK(gotl == wantl, "low %dx%d H=%d W=%d pad=%d tile (%d,%d) pos (%d,%d) cell (%d,%d) ch %d: table %u, rule %u", TH, TW,
                                      a.H, a.W, a.pad_mode, ty, tx, py, px, ly, lx, ch, gotl, wantl);
                            }
                        }
                }
            // elements past the chunk's run (the tail lanes of the last wave-instruction) read zero
            CHECK((w32_off_full<T, CK, false>(a, pl, tab.data(), nullptr, (unsigned)(CK * PSF)) == kOOB), "full tail");
            CHECK((w32_off_low<T, CK, false>(a, pl, tab.data(), nullptr, (unsigned)(CK * PSL)) == kOOB), "low tail");
            // ---- 16-byte pieces ---------------------------------------------------------------------------------------------
            const int Ws = up ? a.W : a.W1, sh = up ? 0 : a.shift1;
            bool inside = true;   // every patch column x0 - 1 .. x0 + TW of the tile inside the source row
            for (int px = 0; px < TW + 2; ++px) inside = inside && x0 + px - 1 - sh >= 0 && x0 + px - 1 - sh < Ws;
            CHECK(w32_x4_ok<T>(a, x0) == inside, "x4 condition %dx%d W=%d W1=%d up=%d shift=%d x0=%d", TH, TW, a.W, a.W1, a.up1, a.shift1, x0);
            if (!T::X4OK || !inside || masked) continue;   // (masked launches stage dword pieces only)
            ++g_x4_tiles;
            for (int ch : chans)
                for (int py = 0; py < PH; ++py)
                    for (int j = 0; j < T::GF; ++j) {
                        const unsigned p4 = w32_off_full4<T, CK>(a, pl, tab.data(), x0, (unsigned)((ch * PH + py) * T::GF + j));
                        for (int k = 0; k < 4 && 4 * j + k < TW + 2; ++k) {
                            const unsigned d = w32_off_full<T, CK, false>(a, pl, tab.data(), nullptr, (unsigned)(ch * PSF + py * PWS + 4 * j + k));
                            CHECK((d == kOOB && p4 == kOOB) || (d != kOOB && p4 != kOOB && p4 + 4u * k == d),
                                  "full x4 %dx%d H=%d W=%d pad=%d up=%d shift=%d x0=%d row %d col %d ch %d: piece %u, dword %u", TH, TW, a.H, a.W,
                                  a.pad_mode, a.up1, a.shift1, x0, py, 4 * j + k, ch, p4, d);
                        }
                    }
            CHECK((w32_off_full4<T, CK>(a, pl, tab.data(), x0, (unsigned)(CK * PH * T::GF)) == kOOB), "full x4 tail");
            if (!up) continue;
            for (int ch : chans)
                for (int py = 0; py < PHL; ++py)
                    for (int j = 0; j < T::GL; ++j) {
                        const unsigned p4 = w32_off_low4<T, CK>(pl, tab.data(), x0, (unsigned)((ch * PHL + py) * T::GL + j));
                        for (int k = 0; k < 4 && 4 * j + k < TW / 2 + 2; ++k) {
                            const unsigned d = w32_off_low<T, CK, false>(a, pl, tab.data(), nullptr, (unsigned)(ch * PSL + py * PWL + 4 * j + k));
                            CHECK((d == kOOB && p4 == kOOB) || (d != kOOB && p4 != kOOB && p4 + 4u * k == d),
                                  "low x4 %dx%d H=%d W=%d pad=%d x0=%d row %d col %d ch %d: piece %u, dword %u", TH, TW, a.H, a.W, a.pad_mode, x0, py,
                                  4 * j + k, ch, p4, d);
                        }
                    }
            CHECK((w32_off_low4<T, CK>(pl, tab.data(), x0, (unsigned)(CK * PHL * T::GL)) == kOOB), "low x4 tail");
        }
}

// maps a few pixels either side of one and two tiles, and the small shapes of profiles/conv_front_end_refactor.md
template <class T, int CK>
static void walk_tile() {
    constexpr int TH = T::TILE_H, TW = T::TILE_W;
    const int hs[] = {5, 6, 7, 9, 12, 14, TH - 1, TH, TH + 1, TH + 2, 2 * TH - 1, 2 * TH, 2 * TH + 1, 2 * TH + 2};
    const int ws[] = {7, 18, 20, 22, 40, TW - 2, TW - 1, TW, TW + 1, TW + 2, TW + 3, 2 * TW - 1, 2 * TW, 2 * TW + 2, 2 * TW + 3};
    for (int H : hs)
        for (int W : ws)
            for (int pad : {WMD_PAD_ZERO, WMD_PAD_REFLECT, WMD_PAD_REPLICATE})
                for (int mode = 0; mode < 3; ++mode) {   // 0: same-size x1, 1: 2x-upsampled x1, 2: data gradient (shift1 = 1)
                    if (H < 3 || W < 3) continue;
                    if (mode == 1 && ((H | W) & 1)) continue;
                    ConvKArgs a;
                    std::memset(&a, 0, sizeof(a));
                    a.H = H, a.W = W, a.pad_mode = pad, a.B = 1;
                    a.up1 = mode == 1 ? 2 : 1, a.shift1 = mode == 2 ? 1 : 0;
                    a.H1 = mode == 1 ? H / 2 : (mode == 2 ? H - 2 : H), a.W1 = mode == 1 ? W / 2 : (mode == 2 ? W - 2 : W);
                    walk_map<T, CK>(a, false);
                    if (mode != 2) walk_map<T, CK>(a, true);
                }
}

int main(int argc, char** argv) {
    const char* which = argc > 1 ? argv[1] : "all";
    const bool all = !std::strcmp(which, "all");
    if (all || !std::strcmp(which, "8x16")) walk_tile<W32QTile<8, 16, 8>, 8>();
    if (all || !std::strcmp(which, "4x32")) walk_tile<W32QTile<4, 32, 8>, 8>();
    if (all || !std::strcmp(which, "6x20")) walk_tile<W32QTile<6, 20, 8>, 8>();
    if (all || !std::strcmp(which, "6x40")) walk_tile<W32Tile<6, 40, 2, 8>, 8>();
    std::printf("checked %ld failed %ld x4_tiles %ld low_cells %ld\n", g_checked, g_failed, g_x4_tiles, g_low);
    return g_failed ? 1 : (g_checked ? 0 : 2);
}
