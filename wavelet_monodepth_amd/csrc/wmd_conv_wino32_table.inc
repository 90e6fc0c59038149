// conv_wino32_kernel instantiations: (TH, TW, WN, CK) = pixel tile, tile groups per block (each two waves: the position
// halves), channels per chunk.  Included by wmd_conv_wino32.hip (explicit instantiation) and by wmd_conv_fwd.hip (configuration table: ConvFamily::Wino32 entries).
WMD_W32_INST(8, 32, 2, 8)     // co32 x 256px, 4 waves, 54 KB of LDS: two blocks per CU
WMD_W32_INST(4, 64, 2, 8)     // co32 x 256px, 4 waves; a tile group = one row of 32 tiles (conflict-free patch reads)
WMD_W32_INST(16, 16, 2, 8)    // co32 x 256px, 4 waves, 16 x 16 tile (80-wide maps)
WMD_W32_INST(6, 40, 2, 8)     // co32 x 240px (60 of 64 tile slots): 40-wide rows, H % 6 == 0 (12x40 ... 96x320 of the 640-wide pyramid)
WMD_W32_INST(8, 16, 1, 8)     // co32 x 128px, 2 waves, 45 KB: three blocks per CU (coarse levels, 80- / 160-wide maps)
WMD_W32_INST(4, 32, 1, 8)     // co32 x 128px, 2 waves, one tile row pair
WMD_W32_INST(8, 64, 4, 8)     // co32 x 512px, 8 waves, 76 KB: one block per CU
WMD_W32_INST(8, 64, 4, 16)    // co32 x 512px, 8 waves, 16-channel chunks (150 KB)
WMD_W32_INST(16, 32, 4, 8)    // co32 x 512px, 8 waves, 16 x 32 tile
WMD_W32_INST(12, 40, 4, 8)    // co32 x 480px (120 of 128 tile slots): a whole 12x40 map per block
// (round 5: 16-channel chunks of the two-group shapes -- <8,32,2,16>, <6,40,2,16>, one block per CU -- measured for the launches
//  that leave one wave per SIMD anyway (L9 / L5 / L1): main loop -5 %, prologue +2 k cycles, launch time unchanged; not kept)
