// conv_wino32q_kernel instantiations: (TH, TW, CK) = pixel tile (one group of 32 Winograd tiles), channels per chunk.
// Included by wmd_conv_wino32q.hip (explicit instantiation) and by wmd_conv_fwd.hip (configuration table: ConvFamily::Wino32Q entries).
WMD_W32Q_INST(8, 16, 8)     // co32 x 128px, 4 quarter-position waves, 47 KB of LDS: three blocks per CU
WMD_W32Q_INST(4, 32, 8)     // co32 x 128px, one tile row pair: 128-byte output lines
WMD_W32Q_INST(6, 20, 8)     // co32 x 120px (30 of 32 tile slots), 45.5 KB: divides every map of the 640x192 pyramid exactly
