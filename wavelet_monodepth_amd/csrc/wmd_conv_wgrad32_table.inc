// conv_wgrad_wino32_kernel instantiations: (TH, TW, WCO, WCI) = pixel tile, 32-channel out / in slabs per block (two waves
// per slab pair).  Included by wmd_conv_wgrad32.hip (explicit instantiation) and by wmd_conv_wgrad.hip (configuration table).
WMD_WG32_INST(2, 32, 2, 2)    // co64 x ci64, 8 waves, 104 KB of LDS
WMD_WG32_INST(2, 32, 1, 4)    // co32 x ci128, 8 waves (Cout = 32 layers)
WMD_WG32_INST(2, 32, 1, 2)    // co32 x ci64, 4 waves
WMD_WG32_INST(2, 40, 2, 2)    // 40-wide rows
WMD_WG32_INST(2, 40, 1, 2)
