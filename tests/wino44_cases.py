"""The case table of the F(4x4,3x3) pins (tests/test_wino44_host.py on the CPU, tests/test_gpu_wino44_pins.py on the GPU): every row is
the smallest shape at which its edge of wmd_conv_wino44_fwd exists.  test_wino44_host.py asserts by predicate on
wino44_ref.dims / blocks that the table reaches every edge."""
import numpy as np


def _case(key, B, C1, C2, Cout, H, W, up1, pad, act="elu", slope=0.0, bias=True):
    return dict(key=key, B=B, C1=C1, C2=C2, Cout=Cout, H=H, W=W, up1=up1, pad=pad, act=act, slope=slope, bias=bias)


TABLE = [
    # the GEMM's grid and reduction (8x8, Cout 32: one block, NTp = 32 < 64 and < 128): chunks on the full / the short positions
    _case("one_block", 1, 32, 0, 32, 8, 8, 1, "reflect"),                     # 1 / -
    _case("chunks_2_1", 1, 32, 32, 32, 8, 8, 2, "reflect"),                   # 2 / 1
    _case("chunks_3_1", 1, 64, 32, 32, 8, 8, 2, "zero", "leaky", 0.1),        # 3 / 1
    _case("chunks_5_3", 1, 40, 72, 32, 8, 8, 2, "replicate"),                 # 5 / 3, dead channels above 32 in both operands
    _case("chunks_16", 1, 512, 0, 32, 8, 8, 1, "reflect"),                    # 16 / -
    # 147 tiles, NTp 160: nbn_long 3, nbn_short 2, NTp % 64 = 32, NT % 32 = 19, th tw = 49; Coutp 96: nbm 2, ragged second block
    _case("tiles_147", 3, 40, 8, 72, 28, 28, 2, "replicate", "leaky", 0.1),
    _case("cout_65", 2, 1, 0, 65, 7, 9, 1, "zero", "none"),                   # one live channel of 32; H, W = 3, 1 mod 4
    _case("up2_no_skip", 2, 16, 0, 32, 12, 20, 2, "reflect"),                 # no chunk at the 11 short positions: M = 0 there
    _case("up1_8x12", 2, 16, 0, 40, 8, 12, 1, "replicate"),                   # H, W = 0 mod 4
    _case("up1_skip_6x10", 2, 16, 8, 32, 6, 10, 1, "reflect"),                # H, W = 2 mod 4; a skip tensor beside a full-resolution x1
    _case("up2_12x20", 2, 16, 24, 19, 12, 20, 2, "zero"),                     # up2, H, W = 0 mod 4
    _case("vec_6x8", 2, 16, 24, 32, 6, 8, 2, "reflect"),                      # 16-byte stores (W % 4 = 0) with a ragged last tile row
    # one row, one column: reflect padding does not exist there
    _case("row_1x9_zero", 2, 8, 0, 8, 1, 9, 1, "zero"),
    _case("row_1x9_replicate", 2, 8, 0, 8, 1, 9, 1, "replicate"),
    _case("col_7x1_zero", 2, 8, 0, 8, 7, 1, 1, "zero"),
    _case("col_7x1_replicate", 2, 8, 0, 8, 7, 1, 1, "replicate"),
]
# H = 2 (and W = 2) under up2: the low-resolution line is one sample, every neighbour is clamped or 0
TABLE += [_case("up2_%dx%d_%s" % (H, W, pad), 2, 8, 8, 8, H, W, 2, pad) for H, W in ((2, 2), (2, 6)) for pad in ("reflect", "zero", "replicate")]
# every activation and bias = NULL, on an up+skip layer (6x10: H, W = 2 mod 4) and on a pure one (5x7: H, W = 1, 3 mod 4)
TABLE += [_case("act_up2_%s" % act, 2, 16, 24, 19, 6, 10, 2, pad, act, 0.1 if act == "leaky" else 0.0)
          for act, pad in (("none", "reflect"), ("elu", "zero"), ("leaky", "replicate"), ("sigmoid", "reflect"))]
TABLE += [_case("act_up1_%s" % act, 1, 24, 0, 8, 5, 7, 1, pad, act, 0.1 if act == "leaky" else 0.0)
          for act, pad in (("none", "replicate"), ("elu", "reflect"), ("leaky", "zero"), ("sigmoid", "replicate"))]
TABLE += [_case("nobias_up2", 2, 16, 24, 19, 6, 10, 2, "replicate", "elu", bias=False),
          _case("nobias_up1", 1, 24, 0, 8, 5, 7, 1, "zero", "sigmoid", bias=False)]

CASES = {c["key"]: c for c in TABLE}
KEYS = [c["key"] for c in TABLE]
assert len(CASES) == len(TABLE)
REPEAT = ("tiles_147", "chunks_16")      # launched twice: bit-identical V, M and y


def operands(c):
    """-> x1, w, bias or None, x2 or None (float32, seeded by the row): weights scaled by sqrt(2 / (9 C))"""
    r = np.random.default_rng(4400 + KEYS.index(c["key"]))
    C = c["C1"] + c["C2"]
    x1 = r.standard_normal((c["B"], c["C1"], c["H"] // c["up1"], c["W"] // c["up1"])).astype(np.float32)
    x2 = r.standard_normal((c["B"], c["C2"], c["H"], c["W"])).astype(np.float32) if c["C2"] else None
    w = (r.standard_normal((c["Cout"], C, 3, 3)) * (2.0 / (9 * C)) ** 0.5).astype(np.float32)
    b = (0.1 * r.standard_normal(c["Cout"])).astype(np.float32)
    return x1, w, (b if c["bias"] else None), x2
