// Staging front end of the two 32x32x2 Winograd trunk kernels: conv_wino32_kernel (wmd_conv_wino32.hip, position halves) and
// conv_wino32q_kernel (wmd_conv_wino32q.hip, position quarters).  Everything ahead of their main loops is one piece of code, the
// wave index a parameter: the block -> (tile, slab, ticket) decode, the out-mask tile-activity test, the folded row / column
// tables, the flattened gather offsets, the descriptors, the LDS-DMA pieces of a chunk, the walk over a block's chunks and the
// activation dispatch of the epilogues.  The pieces are cut where conv_wino32_kernel's cycle stamps 1-6 sit (-DWMD_STAMPS).
// What serves one kernel only stays in its file: the per-channel GENERIC staging of conv_wino32_kernel, the main loops, the
// transforms, the epilogues' exchange and store code.
// The offset arithmetic (w32_full_rc .. w32_off_low4) is __host__ __device__: tests/wino32_stage_host.cpp walks it on the CPU
// against the per-position rule of the GENERIC staging.
#pragma once
#include "wmd_conv_common.h"

namespace wmd {

constexpr unsigned kOOB = 0x80000000u;   // >= any num_records: the descriptor's range check returns 0

__host__ __device__ __forceinline__ unsigned w32_mul24(unsigned x, unsigned y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(x, y);
#else
    return x * y;
#endif
}

// ---- the block's work item ----------------------------------------------------------------------------------------------------
struct W32Item {
    int b, y0, x0;   // frame and first pixel of the TH x TW tile
    int by;          // 32-out-channel slab
    int tick;        // index of the (pixel tile, slab) item's split-K ticket counter (splitk_ticket_finish)
    int ks_n, cps;   // K slices of the launch and chunks per slice (LIST: chosen on the device from the list's length)
    bool none;       // LIST: a block beyond the list or its K split -- nothing to do
};
// The four grid forms.  LIST: the work-list form -- the block's tile comes out of a compacted list of active tiles
// (wmd_conv_args.out_tiles).
template <class T, bool LIST>
__device__ __forceinline__ W32Item w32_item(const ConvKArgs& a) {
    W32Item it;
    int t;
    it.ks_n = a.ksplit, it.cps = a.chunks_per_split, it.none = false;
    if constexpr (LIST) {
        const int n_items = list_total(a.tile_count, a.B) * a.cob;
        it.none = true;
        if ((int)blockIdx.x >= n_items) return it;
        list_ksplit(n_items, a.nchunks, a.ksmax, a.list_slots, it.ks_n, it.cps);
        if ((int)blockIdx.z >= it.ks_n) return it;
        it.none = false;
        const int item = xcd_contiguous(blockIdx.x, n_items);
        const int ti = item / a.cob;
        it.by = item - ti * a.cob;
        t = list_entry(a.tile_list, a.tile_count, a.B, a.tiles_x * a.tiles_y, ti);
        it.tick = item;
    } else if (a.cob > 0) {   // (pixel tile, out-channel slab) items, slab fastest, one contiguous run per XCD (see conv_fwd_kernel)
        const int item = xcd_contiguous(blockIdx.x, gridDim.x);
        t = item / a.cob;
        it.by = item - t * a.cob;
        it.tick = item;
    } else if (a.xcd_slab) {
        // 2-D grid, one out-channel slab per XCD (round 6): workgroup L of a z-slice runs on XCD L % 8 (tools/probes/xcc_probe.hip), so
        // slab L % nslab with nslab a multiple of 8 keeps a slab's 1/nslab of the weight image in ONE L2 instead of streaming the whole
        // image into all eight (counters: L0 / L1 of config 2 read inputs + 8 x 8.4 MB of weights per launch, profiles/r06_notes.md)
        const int L = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y;
        it.by = L % (int)gridDim.y;
        t = L / (int)gridDim.y;
        it.tick = t * (int)gridDim.y + it.by;
    } else {
        t = xcd_contiguous(blockIdx.x, gridDim.x);
        it.by = blockIdx.y;
        it.tick = t * (int)gridDim.y + it.by;
    }
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y;
    it.b = t / a.tiles_y;
    it.y0 = ty * T::TILE_H, it.x0 = tx * T::TILE_W;
    return it;
}

// Block-sparse: true when the tile holds no pixel of out_mask, so that it keeps its zeros.  The caller does not `return` on it: an
// early exit ahead of the pipelined body costs the DENSE launches of this same instantiation 45 % (L14: 110 -> 160 us, A/B builds
// on one box; the epilogue's mask code costs nothing) -- the skipped block walks an empty chunk range and stores nothing instead
// (prologue + an epilogue over zeros: a few thousand cycles against ~50 k for a computed tile).
// flags: one int of LDS per wave.  Contains a barrier: called by every thread of the block.
template <class T>
__device__ __forceinline__ bool w32_tile_inactive(const ConvKArgs& a, int b, int y0, int x0, int* flags, int wave) {
    constexpr int TH = T::TILE_H, TW = T::TILE_W;
    const int tid = threadIdx.x, H = a.H, W = a.W;
    int any = 0;
    for (int i = tid; i < TH * TW; i += T::NT) {
        const int yy = y0 + i / TW, xx = x0 + i % TW;
        if (yy < H && xx < W) any |= a.out_mask[(size_t)b * H * W + (size_t)yy * W + xx];
    }
    // (a ballot per wave + flags in LDS; __syncthreads_or pulls in the device library's work-group reduction)
    const bool wave_any = __builtin_amdgcn_ballot_w64(any != 0) != 0;
    if ((tid & 63) == 0) flags[wave] = wave_any ? 1 : 0;
    __syncthreads();
    int all = 0;
#pragma unroll
    for (int w = 0; w < T::NW; ++w) all |= flags[w];
    return __builtin_amdgcn_readfirstlane(all) == 0;
}

// ---- offset arithmetic (host-callable) ----------------------------------------------------------------------------------------
// The full-resolution chunks of a pure layer all have one geometry: the skip tensor's when x1 is upsampled (x1 then takes the
// low-resolution path), else x1's own (a skip tensor beside a non-upsampled x1 has the same H x W).  The pad / bounds logic is
// separable: PH + PWS (+ PHL + PWL) threads fold one patch row or column each into a byte offset (or -1: reads zero) in a corner
// of LDS, and every flattened element is then channel * plane + row + column: ~20 instructions per element instead of ~80.
// (Round 5 measured the alternative -- every element folding its own row and column, no LDS table, no barrier: 40 VALU
//  instructions per element instead of two table reads.  Slower: offsets phase 3.4 k -> 4.4 k cycles on L14, 2.8 k -> 6.5 k on
//  the 40-wide tiles; a young wave's VALU instructions get the issue slots its SIMD partner's main loop leaves over, so the
//  prologue's price is its VALU count.  s_setprio 1 through the prologue and / or the epilogue: no change either.
//  profiles/r05_stamps.txt, profiles/r05_notes.md.)
struct W32Planes {
    size_t plane1, plane2;   // pixels of one channel plane of x1 / of x2 and the output
    unsigned pb1, pb2;       // ... in bytes
};
__host__ __device__ __forceinline__ W32Planes w32_planes(const ConvKArgs& a) {
    W32Planes p;
    p.plane1 = (size_t)a.H1 * a.W1, p.plane2 = (size_t)a.H * a.W;
    p.pb1 = (unsigned)(p.plane1 * 4), p.pb2 = (unsigned)(p.plane2 * 4);
    return p;
}
// folded byte offset of full-resolution patch row / column t of the tile at (y0, x0) inside a channel plane (-1: reads zero)
__host__ __device__ __forceinline__ int w32_full_rc(const ConvKArgs& a, int y0, int x0, bool row, int t) {
    const bool up = a.up1 == 2;
    const int Hs = up ? a.H : a.H1, Ws = up ? a.W : a.W1, sh = up ? 0 : a.shift1;
    const int g0 = row ? y0 + t - 1 : x0 + t - 1, n = row ? a.H : a.W, ns = row ? Hs : Ws;
    int ok = (int)(g0 <= n);
    const int g = pad_fold(a.pad_mode, g0, n, ok) - sh;
    ok &= (int)(g >= 0) & (int)(g < ns);
    return ok ? (row ? g * Ws * 4 : g * 4) : -1;
}
// Low-resolution halo patch of the upsampled operand: position (py, px) is source pixel (y0/2 - 1 + py, x0/2 - 1 + px).
// The full-resolution pad ring (row -1 / row H) maps onto it as: reflect (-1 -> 1, H -> H-2) and replicate both land in
// the border source pixel, zero padding stays zero; rows beyond the ring (tile overhang) are never used by a stored output.
__host__ __device__ __forceinline__ int w32_low_rc(const ConvKArgs& a, int y0, int x0, bool row, int t) {
    const int s0 = row ? (y0 >> 1) - 1 + t : (x0 >> 1) - 1 + t, n = row ? a.H1 : a.W1;
    const int sc = min(max(s0, 0), n - 1);
    const int ok = (int)(s0 <= n) & ((int)(a.pad_mode != WMD_PAD_ZERO) | (int)(sc == s0));
    return ok ? (row ? sc * a.W1 * 4 : sc * 4) : -1;
}
// entry t of the table: [PH rows][PWS columns] of the full-resolution patch, then [PHL][PWL] of the low-resolution one
template <class T>
__host__ __device__ __forceinline__ void w32_tab_entry(const ConvKArgs& a, int y0, int x0, int* tab, int t) {
    constexpr int PH = T::PH, PWS = T::PWS, PHL = T::PHL, PWL = T::PWL;
    if (t < PH + PWS) tab[t] = w32_full_rc(a, y0, x0, t < PH, t < PH ? t : t - PH);
    else if (t < PH + PWS + PHL + PWL) {
        t -= PH + PWS;
        tab[PH + PWS + t] = w32_low_rc(a, y0, x0, t < PHL, t < PHL ? t : t - PHL);
    }
}
// 16-byte pieces: every used patch column x0 - 1 .. x0 + TW (minus the shift of a data-gradient launch) inside the source row: no
// column is folded, a row of the patch is one contiguous run of the source row (the upsampled operand's low-resolution
// patch likewise: (x0 >> 1) - 1 .. (x0 + TW) >> 1).  Border tiles keep the dword pieces with their per-column folds.
template <class T>
__host__ __device__ __forceinline__ bool w32_x4_ok(const ConvKArgs& a, int x0) {
    const bool up = a.up1 == 2;
    const int Ws = up ? a.W : a.W1, sh = up ? 0 : a.shift1;
    return x0 - 1 - sh >= 0 && x0 + T::TILE_W - sh < Ws && !a.no_x4;
}
// Byte offset of element e of a chunk's flattened [channel][position] run (kOOB: reads zero), dword pieces: full-resolution
// and low-resolution run.  MASKED: block-sparse input support -- a masked position gathers from the out-of-range offset like a
// zero-padded one; mask_b: the frame's plane of in_mask, or null.
template <class T, int CK, bool MASKED>
__host__ __device__ __forceinline__ unsigned w32_off_full(const ConvKArgs& a, const W32Planes& pl, const int* tab, const uint8_t* mask_b, unsigned e) {
    constexpr int PH = T::PH, PWS = T::PWS, PSF = T::PSF;
    const unsigned pbs = a.up1 == 2 ? pl.pb2 : pl.pb1;
    const unsigned ch = e / PSF, pos = e - w32_mul24(ch, PSF);
    const unsigned py = pos / PWS, px = pos - w32_mul24(py, PWS);
    const int r = tab[py], c = tab[PH + px];
    bool ok = ch < CK && (r | c) >= 0;
    // the full-resolution geometry is the mask's own (wino32_pure), so the folded pixel offset indexes it directly
    if (MASKED && mask_b && ok) ok = mask_b[(unsigned)(r + c) >> 2] != 0;
    return ok ? ch * pbs + (unsigned)(r + c) : kOOB;
}
template <class T, int CK, bool MASKED>
__host__ __device__ __forceinline__ unsigned w32_off_low(const ConvKArgs& a, const W32Planes& pl, const int* tab, const uint8_t* mask_b, unsigned e) {
    constexpr int PH = T::PH, PWS = T::PWS, PHL = T::PHL, PWL = T::PWL, PSL = T::PSL;
    const unsigned ch = e / PSL, pos = e - w32_mul24(ch, PSL);
    const unsigned py = pos / PWL, px = pos - w32_mul24(py, PWL);
    const int r = tab[PH + PWS + py], c = tab[PH + PWS + PHL + px];
    bool ok = ch < CK && (r | c) >= 0;
    if (MASKED && mask_b && a.up1 == 2 && ok) {   // 2x2-constant mask (wino32_pure): source pixel (sy, sx) is masked like (2sy, 2sx)
        const unsigned sidx = (unsigned)(r + c) >> 2, sy = sidx / (unsigned)a.W1, sx = sidx - sy * (unsigned)a.W1;
        ok = mask_b[(size_t)(2 * sy) * a.W + 2 * sx] != 0;
    }
    return ok ? ch * pl.pb1 + (unsigned)(r + c) : kOOB;
}
// ... and of 16-byte piece e (w32_x4_ok tiles: four consecutive columns of one patch row)
template <class T, int CK>
__host__ __device__ __forceinline__ unsigned w32_off_full4(const ConvKArgs& a, const W32Planes& pl, const int* tab, int x0, unsigned e) {
    constexpr int PH = T::PH, GF = T::GF;
    const bool up = a.up1 == 2;
    const int sh = up ? 0 : a.shift1;
    const unsigned pbs = up ? pl.pb2 : pl.pb1;
    const unsigned ch = e / (PH * GF), rem = e - w32_mul24(ch, PH * GF);
    const unsigned py = rem / GF, j = rem - w32_mul24(py, GF);
    const int r = tab[min(py, (unsigned)PH - 1)];
    const bool ok = ch < CK && r >= 0;
    return ok ? ch * pbs + (unsigned)r + (unsigned)(x0 - 1 - sh + 4 * (int)j) * 4u : kOOB;
}
template <class T, int CK>
__host__ __device__ __forceinline__ unsigned w32_off_low4(const W32Planes& pl, const int* tab, int x0, unsigned e) {
    constexpr int PH = T::PH, PWS = T::PWS, PHL = T::PHL, GL = T::GL;
    const unsigned ch = e / (PHL * GL), rem = e - w32_mul24(ch, PHL * GL);
    const unsigned py = rem / GL, j = rem - w32_mul24(py, GL);
    const int r = tab[PH + PWS + min(py, (unsigned)PHL - 1)];
    const bool ok = ch < CK && r >= 0;
    return ok ? ch * pl.pb1 + (unsigned)r + (unsigned)((x0 >> 1) - 1 + 4 * (int)j) * 4u : kOOB;
}

// ---- staging state of a block -------------------------------------------------------------------------------------------------
struct ChunkSrc {   // pure layers: the chunk's descriptor and scalar byte base, resolved once per chunk
    __amdgpu_buffer_rsrc_t r;
    unsigned base;
};

// T: W32Tile / W32QTile.  FLAT: every chunk of CK channels lies inside one source tensor.  The chunk's patch is staged as ONE
//   flattened [channel][position] run: every LDS-DMA instruction moves 64 consecutive dwords of it from per-lane offsets that are
//   fixed for the whole layer (channel x plane + gathered position), the chunk is a scalar base -- no per-piece predication,
//   channel arithmetic or branches in the MFMA stream; the upsampled operand takes the structured low-resolution path.
//   FLAT = false (conv_wino32_kernel's GENERIC instantiation) uses the descriptors and the weight pieces only.
// MASKED: the gather offsets test in_mask; dword pieces only (the mask is per position).
template <class T, int CK, bool FLAT, bool MASKED>
struct W32Stage {
    static constexpr int NT = T::NT, PSF = T::PSF, PSL = T::PSL;
    // elements tid + i * NT of a chunk's flattened runs; wave-instructions per chunk and wave: whole 64-dword runs (the tail lanes
    // of the last one carry the out-of-range offset and write zeros into the buffer's padding)
    static constexpr int NPF = FLAT ? (CK * PSF + NT - 1) / NT : 1, NPL = FLAT ? (CK * PSL + NT - 1) / NT : 1;
    // 16-byte pieces (dense flattened staging, tiles whose patch columns all lie inside the source rows): groups per thread
    static constexpr bool X4 = FLAT && !MASKED && T::X4OK;
    static constexpr int NPF4 = (CK * PSF / 4 + NT - 1) / NT, NPL4 = (CK * PSL / 4 + NT - 1) / NT;

    const ConvKArgs& a;
    float* const lds;   // the kernel's LDS: [staging buffers: T::LDS_FLOATS][row / column tables: T::TAB_FLOATS][flags]
    const int wave;
    const bool upl;     // structured low-resolution path of the upsampled operand
    bool x4 = false;
    const W32Planes pl;
    unsigned obF[NPF], obL[NPL], aoff[T::NAV];
    __amdgpu_buffer_rsrc_t r1, r2, rw;
#ifdef WMD_STAMPS
    int c_first = 0;   // the block's first chunk (timing experiments)
#endif

    __device__ __forceinline__ W32Stage(const ConvKArgs& a_, float* lds_, int wave_)
        : a(a_), lds(lds_), wave(wave_), upl(FLAT && a_.up1 == 2), pl(w32_planes(a_)) {}

    __device__ __forceinline__ int* tab() const { return reinterpret_cast<int*>(lds + T::LDS_FLOATS); }

    // row / column tables in LDS (contains a barrier)
    __device__ __forceinline__ void fill_tables(const W32Item& it) {
        w32_tab_entry<T>(a, it.y0, it.x0, tab(), threadIdx.x);
        __syncthreads();
    }
    // per-lane gather offsets of the flattened runs
    __device__ __forceinline__ void gather_offsets(const W32Item& it) {
        const int tid = threadIdx.x;
        const int* tb = tab();
        // (the frame's mask plane is resolved here, once: an index built from the frame number inside the per-element mask branches
        //  becomes a value of divergent control flow, and everything later derived from the frame number -- the split-K finish's
        //  descriptors -- would be treated as varying per lane)
        const uint8_t* mask_b = MASKED && a.in_mask ? a.in_mask + (size_t)it.b * pl.plane2 : nullptr;
        if constexpr (X4) x4 = w32_x4_ok<T>(a, it.x0);
        if (X4 && x4) {
#pragma unroll
            for (int i = 0; i < NPF; ++i) obF[i] = i < NPF4 ? w32_off_full4<T, CK>(a, pl, tb, it.x0, tid + i * NT) : kOOB;
#pragma unroll
            for (int i = 0; i < NPL; ++i) obL[i] = i < NPL4 ? w32_off_low4<T, CK>(pl, tb, it.x0, tid + i * NT) : kOOB;
            // (both arms write every element: were the last stores of the two arms at different indices, the optimizer would merge
            //  them into one store through a selected address and the arrays would live in scratch)
        } else {
#pragma unroll
            for (int i = 0; i < NPF; ++i) obF[i] = w32_off_full<T, CK, MASKED>(a, pl, tb, mask_b, tid + i * NT);
#pragma unroll
            for (int i = 0; i < NPL; ++i) obL[i] = w32_off_low<T, CK, MASKED>(a, pl, tb, mask_b, tid + i * NT);
        }
    }
    // descriptors of the frame's two sources and of the weight image; weights: the slab's two 16-channel runs of a chunk as
    // 16-byte pieces; piece e -> run e / (CK*64), slot e % (CK*64)
    __device__ __forceinline__ void sources(const W32Item& it) {
        const int tid = threadIdx.x;
        const float* x1b = a.x1 + (size_t)it.b * a.C1 * pl.plane1;
        const float* x2b = a.x2 ? a.x2 + (size_t)it.b * a.C2 * pl.plane2 : a.x1;
        r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x1b), 0, (int)(a.C1 * pl.plane1 * 4), 0x00020000);
        r2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x2b), 0, (int)(a.C2 * pl.plane2 * 4), 0x00020000);
        rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.wp), 0, (int)((size_t)a.ncot * a.nci4 * 16 * 64 * 4), 0x00020000);
#pragma unroll
        for (int v = 0; v < T::NAV; ++v) {
            const int e = tid + v * NT;
            const int run = e / (CK * 64), rem = e % (CK * 64);
            const int cot = min(it.by * 2 + run, a.ncot - 1);
            aoff[v] = e < 2 * CK * 64 ? (unsigned)(((size_t)cot * a.nci4 * 16 * 64 + (size_t)rem * 4) * 4) : kOOB;
        }
    }

    // Chunk kinds: UP = CK channels of the upsampled x1, staged at low resolution (pure layers only); FULL = anything else.
    __device__ __forceinline__ bool is_up(int chunk) const { return upl && (chunk + 1) * CK <= a.C1; }
    // end of the block's UP chunks in [c_begin, c_end)
    __device__ __forceinline__ int up_end(int c_begin, int c_end) const { return min(c_end, max(c_begin, upl ? a.C1 / CK : 0)); }
    __device__ __forceinline__ ChunkSrc chunk_src(int chunk) const {
        ChunkSrc cs;
        const int ci0 = chunk * CK;
        const bool in1 = ci0 < a.C1;
        cs.r = in1 ? r1 : r2;
        cs.base = in1 ? (unsigned)ci0 * pl.pb1 : (unsigned)(ci0 - a.C1) * pl.pb2;
        return cs;
    }
    // One wave-instruction each: piece v of the chunk's weights, piece q of its full-resolution / low-resolution patch run into
    // the staging buffer bufp.  stage_full_piece / stage_up_piece: the patch pieces, then the weight pieces.
    __device__ __forceinline__ void stage_weight_piece(int chunk, float* bufp, int v) const {
#ifdef WMD_STAMPS
        if ((a.dbg_mode & 4) && chunk > c_first + 1) return;   // timing experiment: no weight traffic after the first two chunks (results wrong)
#endif
        const unsigned soffA = (unsigned)chunk * (unsigned)(T::RUN * 4);
        const int e0 = wave * 64 + v * NT;   // first piece of this wave-instruction (a multiple of 64: inside one run)
        if (T::NAV * NT == 2 * CK * 64 || e0 < 2 * CK * 64)   // wave-uniform: whole wave-instructions only
            lds_dma16(rw, (lds_ptr_t)(bufp + T::B_FLOATS + (e0 / (CK * 64)) * T::RUN_LDS + (e0 % (CK * 64)) * 4), aoff[v], soffA);
    }
    __device__ __forceinline__ bool dbg_no_patch(int chunk) const {
#ifdef WMD_STAMPS
        return (a.dbg_mode & 8) && chunk > c_first + 1;   // timing experiment: no patch traffic either
#else
        return false;
#endif
    }
    __device__ __forceinline__ void stage_full_patch(float* bufp, int q, const ChunkSrc& cs) const {
        if (X4 && x4) {      // block-uniform: 64 lanes x 16 bytes = 256 consecutive dwords of the chunk's run per instruction
            if (q < NPF4 && ((q + 1) * NT * 4 <= CK * PSF || (wave * 64 + q * NT) * 4 < CK * PSF))
                lds_dma16(cs.r, (lds_ptr_t)(bufp + (wave * 64 + q * NT) * 4), obF[q], cs.base);
        } else if ((q + 1) * NT <= CK * PSF || wave * 64 + q * NT < CK * PSF)   // wave-uniform: skip wholly empty runs
            lds_dma4(cs.r, (lds_ptr_t)(bufp + wave * 64 + q * NT), obF[q], cs.base);
    }
    __device__ __forceinline__ void stage_full_piece(int chunk, float* bufp, int q, const ChunkSrc& cs) const {
        if (q < NPF) {
            if (!dbg_no_patch(chunk)) stage_full_patch(bufp, q, cs);
        } else {
            stage_weight_piece(chunk, bufp, q - NPF);
        }
    }
    __device__ __forceinline__ void stage_up_piece(int chunk, float* bufp, int q) const {
        if (q < NPL) {
            if (dbg_no_patch(chunk)) return;
            if (X4 && x4) {
                if (q < NPL4 && ((q + 1) * NT * 4 <= CK * PSL || (wave * 64 + q * NT) * 4 < CK * PSL))
                    lds_dma16(r1, (lds_ptr_t)(bufp + (wave * 64 + q * NT) * 4), obL[q], (unsigned)(chunk * CK) * pl.pb1);
            } else if ((q + 1) * NT <= CK * PSL || wave * 64 + q * NT < CK * PSL)
                lds_dma4(r1, (lds_ptr_t)(bufp + wave * 64 + q * NT), obL[q], (unsigned)(chunk * CK) * pl.pb1);
        } else {
            stage_weight_piece(chunk, bufp, q - NPL);
        }
    }
    // the block's first chunk into buffer 0; full_piece(chunk, bufp, q, cs): the kernel's FULL piece q of NPB_F + T::NAV
    template <int NPB_F, class FullPiece>
    __device__ __forceinline__ void issue_first(int c_begin, int c_end, FullPiece&& full_piece) {
#ifdef WMD_STAMPS
        c_first = c_begin;
#endif
        if (c_begin < c_end) {
            if (is_up(c_begin)) {
                static_for<NPL + T::NAV>([&](auto qc) { stage_up_piece(c_begin, lds, decltype(qc)::value); });
            } else {
                const ChunkSrc cs0 = chunk_src(c_begin);
                static_for<NPB_F + T::NAV>([&](auto qc) { full_piece(c_begin, lds, decltype(qc)::value, cs0); });
            }
        }
    }
    __device__ __forceinline__ void issue_first(int c_begin, int c_end) {
        issue_first<NPF>(c_begin, c_end, [&](int chunk, float* bufp, int q, const ChunkSrc& cs) { stage_full_piece(chunk, bufp, q, cs); });
    }
};

// body(c, up_tag, next_tag) over the chunks [c_begin, c_end), of which [c_begin, up_end) are UP chunks (HAS_UP):
//   up_tag: false_type = full-resolution chunk, true_type = low-resolution chunk of the upsampled operand
//   next_tag: 0 = last chunk, 1 = the next chunk is FULL, 2 = the next chunk is UP
// Two plain loops (upsampled chunks first, then the rest) with peeled last iterations: one body per loop keeps the
// accumulators in place across the back edge (a single loop that switches between body variants makes the register
// allocator rotate the 128 accumulator registers through copies and spills).
template <bool HAS_UP, class Body>
__device__ __forceinline__ void w32_walk_chunks(int c_begin, int c_end, int up_end, Body&& body) {
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    int c = c_begin;
    if constexpr (HAS_UP) {
        for (; c + 1 < up_end; ++c) body(c, std::true_type{}, I2{});
        if (c < up_end) {
            if (up_end < c_end) body(c, std::true_type{}, I1{});
            else body(c, std::true_type{}, I0{});
            ++c;
        }
    }
    for (; c + 1 < c_end; ++c) body(c, std::false_type{}, I1{});
    if (c < c_end) body(c, std::false_type{}, I0{});
}

// Activation with the kind as a compile-time constant (w32_act / w32_act2, wmd_conv_common.h): the epilogue selects ONE instantiation
// of its store loop per launch (a run-time switch per element put ~100 scalar branches into every wave's epilogue: 12 k -> 5.5 k
// cycles on L14).  act_sel < 0: split-K partial sums, neither bias nor activation.
template <class Store>
__device__ __forceinline__ void w32_act_dispatch(int act_sel, Store&& store) {
    if (act_sel < 0) store(std::integral_constant<int, -1>{});
    else if (act_sel == WMD_ACT_ELU) store(std::integral_constant<int, WMD_ACT_ELU>{});
    else if (act_sel == WMD_ACT_LEAKY) store(std::integral_constant<int, WMD_ACT_LEAKY>{});
    else if (act_sel == WMD_ACT_SIGMOID) store(std::integral_constant<int, WMD_ACT_SIGMOID>{});
    else store(std::integral_constant<int, WMD_ACT_NONE>{});
}

}  // namespace wmd
