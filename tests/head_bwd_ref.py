"""The wavelet heads' backward restated from the header's contract (include/wmd.h: wmd_head3x3_bwd_args, wmd_head1x1_bwd_args) on
oracle.decoder_ref, generic in the dtype of its operands (float64: the oracle; float32: the reference's own rounding), the case
tables of test_gpu_head_bwd.py, and the host rules of the launches re-derived in Python (wmd_head_bwd1.h, wmd_head_bwd.hip), so
that a table row that no longer reaches the form it is there for fails (test_head_bwd_ref_oracle.py, and again on the GPU).

The adjoint of pad + 3x3 and of the 1x1 is torch.autograd over decoder_ref.conv3x3 / conv1x1 -- the padding semantics already pinned
to the reference's goldens.  The gate is the kernels' documented rule on the activation OUTPUT m: m > 0 ? 1 : dslope + delu * m
(none: 1, leaky: the slope, ELU: 1 + m); mid and x are inputs of the calls, so there is no kink ambiguity."""
import zlib

import torch

from oracle import decoder_ref as R

SLOPE = 0.1
ACTS = ("none", "leaky", "elu")
PADS = ("zero", "reflect", "replicate")
# wmd_head_bwd1.h / wmd_head_bwd.hip
HB_WW = H1_WW = 4
HB_MAX_BLK, H1_MAX_BLK = 256, 512
DATA_BLK, DATA_BLK_MERGED = 4096, 1024
HB_PART, H1_PART = 8 * 256 + 16, 16 * 256 + 64
HB_MAX_SLICES = 24


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def randn(g, *shape):
    return torch.randn(shape, generator=g)


def cast(v, dt):
    if isinstance(v, (list, tuple)):
        return [cast(e, dt) for e in v]
    return None if v is None else v.to(dt)


# ---- operands -----------------------------------------------------------------------------------------------------------------
def activation(z, act):
    return z if act == "none" else (torch.nn.functional.leaky_relu(z, SLOPE) if act == "leaky" else torch.nn.functional.elu(z))


def act_output(g, act, *shape):
    """a real activation output of random pre-activations; about 1 % of its elements +0.0 and 1 % -0.0 (both: the <= 0 branch)"""
    m = activation(randn(g, *shape), act).contiguous()
    r = torch.rand(shape, generator=g)
    m[r < 0.01] = 0.0
    m[r > 0.99] = -0.0
    flat = m.view(-1)
    flat[0], flat[-1] = 0.0, -0.0
    return m


def case3x3(tag, B, H, W, Ct, n_out, heads, act):
    """heads: [(row0, nrows, ch0, nch)] -> dy3 [B,n_out,H,W], mid [B,Ct,H,W], w3 per head"""
    g = gen(tag)
    return dict(B=B, H=H, W=W, Ct=Ct, n_out=n_out, heads=list(heads), act=act, dy3=randn(g, B, n_out, H, W) * 0.5,
                mid=act_output(g, act, B, Ct, H, W), w3=[randn(g, nr, nch, 3, 3) / (1.5 * nch ** 0.5) for _r0, nr, _c0, nch in heads])


def case1x1(tag, B, H, W, C, Ct, x_act, dz=True):
    g = gen(tag)
    return dict(B=B, H=H, W=W, C=C, Ct=Ct, x_act=x_act, x=act_output(g, x_act, B, C, H, W), w1=randn(g, Ct, C) / C ** 0.5,
                dz=randn(g, B, Ct, H, W) * 0.5 if dz else None)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def gate(m, act, slope=SLOPE):
    """act'(.) from the activation output m"""
    if act == "none":
        return torch.ones_like(m)
    return torch.where(m > 0, torch.ones_like(m), torch.full_like(m, slope) if act == "leaky" else 1 + m)


def head3x3_bwd(dy3, mid, heads, w3, pad, act, slope=SLOPE):
    """-> dict(dz [B,Ct,H,W] (NaN in the channels of no head), dw3 [per head], db3 [per head])"""
    o = {"dz": torch.full_like(mid, float("nan")), "dw3": [], "db3": []}
    for (row0, nrows, ch0, nch), w in zip(heads, w3):
        m = mid[:, ch0:ch0 + nch].detach().clone().requires_grad_(True)
        wv = w.detach().clone().requires_grad_(True)
        b = torch.zeros(nrows, dtype=mid.dtype, requires_grad=True)
        y = R.conv3x3(m, wv, b, pad)
        dmid, dw, db = torch.autograd.grad(y, (m, wv, b), dy3[:, row0:row0 + nrows].contiguous())
        o["dz"][:, ch0:ch0 + nch] = dmid * gate(m.detach(), act, slope)
        o["dw3"].append(dw)
        o["db3"].append(db)
    return o


def head1x1_bwd(dz, x, w1, x_act, x_slope=SLOPE):
    """-> dict(dx [B,C,H,W], dw1 [Ct,C], db1 [Ct])"""
    Ct, C = w1.shape
    xv = x.detach().clone().requires_grad_(True)
    wv = w1.detach().clone().view(Ct, C, 1, 1).requires_grad_(True)
    b = torch.zeros(Ct, dtype=x.dtype, requires_grad=True)
    dxx, dw, db = torch.autograd.grad(R.conv1x1(xv, wv, b), (xv, wv, b), dz.contiguous())
    return {"dx": dxx * gate(x, x_act, x_slope), "dw1": dw.view(Ct, C), "db1": db}


def oracle3x3(c, pad, dt):
    return head3x3_bwd(cast(c["dy3"], dt), cast(c["mid"], dt), c["heads"], cast(c["w3"], dt), pad, c["act"])


def oracle1x1(c, dt, dz=None):
    return head1x1_bwd(cast(c["dz"], dt) if dz is None else dz, cast(c["x"], dt), cast(c["w1"], dt), c["x_act"])


def oracle_both(c3, c1, pad, dt):
    """both stages in dtype dt, the 1x1 stage on the 3x3 stage's dz (every channel of mid belongs to a head)"""
    o = oracle3x3(c3, pad, dt)
    o.update(oracle1x1(c1, dt, dz=o["dz"]))
    return o


# ---- an independent formulation: explicit loops over the taps and the padded positions that fold onto a pixel ------------------------
def _source(Q, n, pad):
    """the source coordinate the padded coordinate Q (-1 .. n) reads, None beyond the border under zero padding"""
    if 0 <= Q < n:
        return Q
    if pad == "zero":
        return None
    if pad == "replicate":
        return 0 if Q < 0 else n - 1
    return 1 if Q < 0 else n - 2      # reflect (n >= 2)


def _preimages(n, pad):
    """per source coordinate q, the padded coordinates that fold onto it"""
    pre = [[] for _ in range(n)]
    for Q in range(-1, n + 1):
        q = _source(Q, n, pad)
        if q is not None:
            pre[q].append(Q)
    return pre


def head3x3_bwd_loops(dy, mid, w, pad):
    """one head, float64: dy [B,nrows,H,W], mid [B,nch,H,W], w [nrows,nch,3,3] -> (dmid, dw3, db3).  The forward reads
    midpad(p + (ty - 1, tx - 1)), so the padded position Q receives dy(Q - (ty - 1, tx - 1)) through tap (ty, tx)."""
    B, nrows, H, W = dy.shape
    dmid, dw = torch.zeros_like(mid), torch.zeros_like(w)
    ys, xs = _preimages(H, pad), _preimages(W, pad)
    for qy in range(H):
        for qx in range(W):
            for Qy in ys[qy]:
                for Qx in xs[qx]:
                    for ty in range(3):
                        for tx in range(3):
                            py, px = Qy - (ty - 1), Qx - (tx - 1)
                            if 0 <= py < H and 0 <= px < W:
                                d = dy[:, :, py, px]                                            # [B, nrows]
                                dmid[:, :, qy, qx] += d @ w[:, :, ty, tx]                       # [B, nch]
                                dw[:, :, ty, tx] += d.t() @ mid[:, :, qy, qx]                   # [nrows, nch]
    return dmid, dw, dy.sum((0, 2, 3))


# ---- the host rules, re-derived ------------------------------------------------------------------------------------------------
def head_bwd_tiles(B, H, W):
    return B * ((H * W + 63) // 64)


def _grid(tiles, waves, cap):
    return max(1, min((tiles + waves - 1) // waves, cap))


def head3x3_blocks(tiles):
    return _grid(tiles, HB_WW, HB_MAX_BLK)


def head1x1_blocks(tiles):
    return _grid(tiles, H1_WW, H1_MAX_BLK)


def head_bwd_data_blocks(tiles, cap=DATA_BLK):
    return _grid(tiles, 4, cap)


def n_slices(heads):
    return sum((nch + 63) // 64 for _r0, _nr, _c0, nch in heads)


def workspace3x3(B, H, W, heads):
    """-> (what wmd_head3x3_bwd_workspace_floats answers, what the 3x3 stage / the three-launch form needs, what the fused form needs)"""
    t, n = head_bwd_tiles(B, H, W), n_slices(heads)
    nb3, nb1 = head3x3_blocks(t), head1x1_blocks(t)
    return max(nb3, nb1) * n * HB_PART, nb3 * n * HB_PART, nb1 * n * HB_PART


def workspace1x1(B, H, W, C, Ct):
    return head1x1_blocks(head_bwd_tiles(B, H, W)) * ((Ct + 63) // 64) * ((C + 63) // 64) * H1_PART


def head_bwd_fused_ok(B, H, W, heads, Ct, C, pad, with_dx=True, switch=True):
    """head_bwd_fused_ok, for 16-byte aligned operands"""
    if not switch or len(heads) != 2 or Ct != 64 or C != 32 or not with_dx or pad != "reflect":
        return False
    if any(nr != 3 or nch != 32 or c0 not in (0, 32) for _r0, nr, c0, nch in heads) or heads[0][2] == heads[1][2]:
        return False
    if B * 64 * H * W * 4 >= 2 ** 31:
        return False
    return H >= 4 and W >= 4 and W % 4 == 0 and (H * W) % 64 == 0


def _loop(tiles, blocks, waves=4):
    """a persistent loop of `blocks` blocks of `waves` waves over `tiles` tiles -> (whole passes beyond the first, remainder)"""
    per = blocks * waves
    return dict(blocks=blocks, wraps=(tiles - 1) // per, remainder=tiles % per)


def classify(B, H, W):
    """what a (B, H, W) map exercises: 16-pixel groups by the form their gather takes (a group whose sixteen pixels are all two or
    more away from every edge: inner; else tiny when H < 4 or W < 4, else edge), whole and ragged 64-pixel tiles (per frame times B),
    the 16-byte path, and the wraps of each persistent loop"""
    HW = H * W
    tiny = H < 4 or W < 4
    groups = dict(inner=0, edge=0, tiny=0)
    straddle = False
    for P0 in range(0, HW, 16):
        px = range(P0, min(P0 + 16, HW))
        inner = len(px) == 16 and all(2 <= P // W < H - 2 and 2 <= P % W < W - 2 for P in px)
        groups["inner" if inner else ("tiny" if tiny else "edge")] += 1
        straddle |= px[0] // W != px[-1] // W
    tiles = head_bwd_tiles(B, H, W)
    return dict(groups={k: v * B for k, v in groups.items()}, whole=B * (HW // 64), ragged=B * (1 if HW % 64 else 0), vec=HW % 4 == 0, tiny=tiny,
                straddle=straddle, tiles=tiles,
                loops=dict(w3=_loop(tiles, head3x3_blocks(tiles)), w1=_loop(tiles, head1x1_blocks(tiles)),      # weight stages; w1: the fused kernel too
                           d=_loop(tiles, head_bwd_data_blocks(tiles)), d_merged=_loop(tiles, head_bwd_data_blocks(tiles, DATA_BLK_MERGED))))


# ---- the tables of test_gpu_head_bwd.py -------------------------------------------------------------------------------------------
def _two(nch):
    return dict(Ct=2 * nch, n_out=6, heads=[(0, 3, 0, nch), (3, 3, nch, nch)])


_LL = [(0, 1, 0, 16), (1, 3, 16, 64), (4, 3, 80, 64)]
LAYOUTS = {    # name -> Ct, n_out, [(row0, nrows, ch0, nch)] in the order the heads are listed
    "n8": _two(8), "n20": _two(20), "n64": _two(64),
    "n80": _two(80),                                                          # two slices per head; db3 from the first alone
    "ll": dict(Ct=144, n_out=7, heads=_LL),                                   # rows 0 | 1..3 | 4..6
    "ll_reordered": dict(Ct=144, n_out=7, heads=[_LL[2], _LL[0], _LL[1]]),    # listed -, LL, +
    "one": dict(Ct=24, n_out=3, heads=[(0, 3, 0, 24)]),
    "ll_only": dict(Ct=16, n_out=1, heads=[(0, 1, 0, 16)]),                   # the <1> instantiations alone
    "gap": dict(Ct=48, n_out=6, heads=[(0, 3, 0, 16), (3, 3, 24, 16)]),       # channels 16..23 and 40..47 belong to no head
    "s24": dict(Ct=1536, n_out=7, heads=[(0, 1, 0, 512), (1, 3, 512, 512), (4, 3, 1024, 512)]),     # 24 slices: HB_MAX_SLICES
    "s25": dict(Ct=1537, n_out=7, heads=[(0, 1, 0, 512), (1, 3, 512, 512), (4, 3, 1024, 513)]),     # 25: refused
}
CROSSED = ("n8", "n20", "n64", "n80", "ll", "ll_reordered", "one", "gap")     # every one on a tiny, an edge and an inner shape
# (B, H, W) -> what the row is there for (asserted by row_reaches) and the layouts it runs
A_TABLE = [
    ((3, 2, 2), ("tiny", "ragged", "vec", "two_rows"), ("n8", "ll", "gap", "one", "ll_only")),
    ((2, 1, 7), ("tiny", "one_row", "scalar"), ("n20", "ll_reordered")),
    ((2, 5, 1), ("tiny", "one_column", "scalar"), ("n64", "one")),
    ((2, 3, 6), ("tiny", "scalar", "near_4_rows", "both_ring_rows_onto_one"), ("n80", "gap")),
    ((1, 2, 5), ("tiny", "scalar"), ("ll_reordered", "n20")),
    ((2, 5, 7), ("edge", "scalar", "ragged"), ("n8", "n80", "ll", "gap", "ll_only")),
    ((2, 6, 10), ("edge", "vec", "ragged"), ("n20", "n64", "ll_reordered", "one")),
    ((2, 6, 40), ("inner", "edge", "vec", "whole", "ragged", "straddle"), CROSSED + ("ll_only",)),
    ((1, 4, 16), ("edge", "no_inner", "whole", "no_ragged", "vec", "nblk1"), ("n64", "ll")),
    ((129, 8, 64), ("inner", "w3_wraps_rem8"), ("n20", "ll")),
    ((16387, 2, 2), ("tiny", "d_wraps_rem3"), ("n8",)),
]
REDUCE3_TILES = (1, 2, 3, 5, 9, 17)      # frames of 4 x 16 (one tile each): 1, 1, 1, 2, 3 and 5 blocks for the four-way reduce
REDUCE1_TILES = (1, 3, 17, 33)           # 1, 1, 5 and 9 blocks for the sixteen-way reduce

B_CHANNELS = [(8, 8), (24, 16), (32, 64), (80, 72), (130, 136)]      # (C, Ct)
B_SHAPES = [(2, 5, 7), (2, 6, 10), (1, 8, 8), (2, 8, 64)]
B_WRAPS = [((2051, 2, 2), ("w1_wraps_rem3",)), ((16387, 2, 2), ("d_wraps_rem3",))]

C_EXTRA = (4099, 2, 2)                   # nb3 = 256, nb1w = 512, nb1d = 1024: three different blockIdx.x extents in one launch
C_LAYOUT_C = {"n8": 8, "n20": 24, "n64": 32, "n80": 40, "one": 16}     # the three-launch form: layouts of 3-row heads without a gap -> C of x

D_SHAPES = [((1, 4, 16), ("whole", "no_inner", "one_tile")), ((3, 8, 48), ("inner",)), ((2, 24, 40), ("inner", "straddle")),
            ((2051, 4, 16), ("w1_wraps_rem3",))]
D_LAYOUTS = {   # name -> n_out, heads
    "r03": (6, [(0, 3, 0, 32), (3, 3, 32, 32)]), "r03_swapped": (6, [(0, 3, 32, 32), (3, 3, 0, 32)]),
    "r14": (7, [(1, 3, 0, 32), (4, 3, 32, 32)]), "r41_swapped": (7, [(4, 3, 32, 32), (1, 3, 0, 32)]),
}
D_NOT_ADMITTED = [((1, 32, 6), "reflect", True, "W % 4 != 0"), ((1, 4, 8), "reflect", True, "H*W % 64 != 0"), ((1, 4, 16), "zero", True, "zero padding"),
                  ((1, 4, 16), "reflect", False, "dx == NULL")]


def pads_of(shape):
    """the paddings a shape runs under: reflection needs two rows and two columns"""
    return [p for p in PADS if p != "reflect" or (shape[1] >= 2 and shape[2] >= 2)]


def a_runs():
    """every (shape, layout, pad, act) of section A; the activation rotates over the runs"""
    out, i = [], 0
    for shape, _why, layouts in A_TABLE:
        for name in layouts:
            for k, pad in enumerate(pads_of(shape)):
                out.append((shape, name, pad, ACTS[(i + k) % 3]))
            i += 1
    return out


def row_reaches(shape, why):
    """does the (B, H, W) reach every form its table row names?  -> the names it does not reach"""
    B, H, W = shape
    c = classify(B, H, W)
    g, lp = c["groups"], c["loops"]
    test = {
        "tiny": c["tiny"] and g["tiny"] > 0 and g["edge"] == 0, "edge": g["edge"] > 0, "inner": g["inner"] > 0, "no_inner": g["inner"] == 0,
        "ragged": c["ragged"] > 0, "no_ragged": c["ragged"] == 0, "whole": c["whole"] > 0, "vec": c["vec"], "scalar": not c["vec"],
        "straddle": c["straddle"], "one_row": H == 1, "one_column": W == 1, "near_4_rows": H == 3 and W >= 4, "one_tile": c["tiles"] == 1,
        # reflection: row 1 takes ring row -1 and row H - 2 takes ring row H.  H = 2: every row takes one; H = 3: row 1 takes both
        "two_rows": H == 2, "both_ring_rows_onto_one": H == 3,
        "nblk1": lp["w3"]["blocks"] == 1,
        "w3_wraps_rem8": lp["w3"]["wraps"] >= 1 and lp["w3"]["remainder"] == 8, "w1_wraps_rem3": lp["w1"]["wraps"] >= 1 and lp["w1"]["remainder"] == 3,
        "d_wraps_rem3": lp["d"]["wraps"] >= 1 and lp["d"]["remainder"] == 3,
    }
    return [k for k in why if not test[k]]
