"""wmd_sparse_conv restated (include/wmd.h, at wmd_sparse_conv_args): a plain oracle in float64 or float32, a mirror of the
host's choice of instantiation, and the case table of tests/test_gpu_sparse_conv.py.  CPU only; nothing here calls the library
or its wrappers, and the oracle uses no F.conv2d: it walks the listed pixels and the taps, as the C ABI words it.

    for every listed pixel p (the first min(nnz, max_out) entries of out_coords) and every output channel
        for every tap: fold the coordinate through the padding (reflect folds, zero drops the tap); the tap contributes only
                       where in_mask at the folded fine coordinate is non-zero (3x3 only; NULL = everywhere); the source is
                       x1[c1_off : c1_off + C1] at (y // up1, x // up1) followed by x2 at (y, x)
        y[co, p] = out_scale * act(sum + bias)        dual: - out_scale * act(the same with w2, bias2 over the slice c1_off2)
    pixels that are not listed are returned as NaN."""
import zlib

import torch

NAN = float("nan")


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def _fold(g, n, pad):
    """a padded coordinate in [-1, n] -> (source coordinate, the tap is alive)"""
    alive = torch.ones_like(g, dtype=torch.bool)
    if pad == "reflect":
        g = torch.where(g < 0, -g, g)
        g = torch.where(g >= n, 2 * n - 2 - g, g)
    elif pad == "replicate":
        g = g.clamp(0, n - 1)
    else:
        assert pad == "zero", pad
        alive = (g >= 0) & (g < n)
    return g.clamp(0, n - 1), alive


def _act(v, act, slope):
    if act == "elu":
        return torch.where(v > 0, v, torch.expm1(v))
    if act == "leaky":
        return torch.where(v > 0, v, v * slope)
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-v))
    assert act in ("none", None), act
    return v


def _frame(x1, x2, in_mask, coords, nnz, max_out, H, W, ksize, dtype, up1, pad, act, slope, out_scale, C1, heads):
    Cout = heads[0][0].shape[0]
    y = torch.full((Cout, H, W), NAN, dtype=dtype)
    n = max(0, min(int(nnz), int(max_out)))
    if n == 0:
        return y
    p = coords.reshape(-1)[:n].long()
    assert int(p.min()) >= 0 and int(p.max()) < H * W, "a listed pixel outside the map"
    oy, ox = p // W, p % W
    r = ksize // 2
    out = None
    for w, b, off in heads:
        acc = torch.zeros((Cout, n), dtype=dtype)
        for ky in range(-r, r + 1):
            for kx in range(-r, r + 1):
                gy, ay = _fold(oy + ky, H, pad) if ksize == 3 else (oy, torch.ones_like(oy, dtype=torch.bool))
                gx, ax = _fold(ox + kx, W, pad) if ksize == 3 else (ox, torch.ones_like(ox, dtype=torch.bool))
                on = ay & ax
                if ksize == 3 and in_mask is not None:
                    on = on & (in_mask[gy, gx] != 0)
                src = x1[off:off + C1][:, gy // up1, gx // up1]
                if x2 is not None:
                    src = torch.cat([src, x2[:, gy, gx]], 0)
                src = torch.where(on[None], src.to(dtype), torch.zeros((), dtype=dtype))     # selected, never multiplied
                acc = acc + w[:, :, ky + r, kx + r].to(dtype) @ src
        if b is not None:
            acc = acc + b.to(dtype)[:, None]
        v = _act(acc, act, slope) * out_scale
        out = v if out is None else out - v
    y[:, oy, ox] = out
    return y


def sparse_conv_oracle(x1, w, b, coords, nnz, max_out, H, W, ksize, dtype, x2=None, up1=1, in_mask=None, pad="reflect", act="none",
                       slope=0.0, out_scale=1.0, c1=None, c1_off=0, w2=None, b2=None, c1_off2=0):
    """x1 [C1tot,H/up1,W/up1], x2 [C2,H,W] or None, in_mask [H,W] or None, coords [>= max_out] int, nnz an int -> y [Cout,H,W] in
    `dtype`, NaN at the pixels that are not listed.  Batched: one more leading dimension on x1 / x2 / in_mask / coords, nnz a
    sequence of B counts -> y [B,Cout,H,W]."""
    assert dtype in (torch.float64, torch.float32) and ksize in (1, 3) and up1 in (1, 2)
    C1 = x1.shape[-3] if c1 is None else c1
    assert w.shape[1] == C1 + (0 if x2 is None else x2.shape[-3]) and w.shape[2] == ksize
    heads = [(w, b, c1_off)] + ([(w2, b2, c1_off2)] if w2 is not None else [])
    if x1.dim() == 3:
        return _frame(x1, x2, in_mask, coords, nnz, max_out, H, W, ksize, dtype, up1, pad, act, slope, out_scale, C1, heads)
    return torch.stack([_frame(x1[f], None if x2 is None else x2[f], None if in_mask is None else in_mask[f], coords[f], nnz[f], max_out,
                               H, W, ksize, dtype, up1, pad, act, slope, out_scale, C1, heads) for f in range(x1.shape[0])])


# ---- the host's choice of instantiation, restated (wmd_sparse_conv) ------------------------------------------------------------------
def select(B, H, W, up1, Cout, ksize, max_out, dual=False, grid_target=2048, rows_on=True, mr_force=0):
    """-> the instantiation wmd_sparse_conv launches for a problem and its grid: three of the host's rules --
    MR doubles while tiles * B * ceil(ncot / MR) > 512, capped by ncot and 4; ROWS needs 3x3, W >= 3 and W / up1 >= 3;
    grid.x = max(1, min(tiles, grid_target / (groups * B))).  A dual launch is the MR = 1 instantiation of its family."""
    ncot, tiles = -(-Cout // 16), -(-max_out // 16)
    MR = 1
    while MR < 4 and MR < ncot and tiles * B * -(-ncot // MR) > 512:
        MR *= 2
    if mr_force in (1, 2, 4):
        MR = min(mr_force, 4 if ncot >= 4 else 2 if ncot >= 2 else 1)
    if dual:
        MR = 1
    taps = 9 if ksize == 3 else 1
    rows = taps == 9 and W >= 3 and W // up1 >= 3 and rows_on
    WK, UN = (8, 2) if taps == 9 else (4, 8)
    groups = -(-ncot // MR)
    return dict(name="sparse_conv_kernel<%d,%d,%s,%d,%d,%s>" % (MR, taps, "true" if dual else "false", WK, UN, "true" if rows else "false"),
                MR=MR, WK=WK, ncot=ncot, groups=groups, tiles=tiles, grid_x=max(1, min(tiles, grid_target // (groups * B))))


def k_slices(ntile, WK, split_waves=2048):
    """S, the K slices per tile the device picks from a frame's tile count: K is merged only while ntile * S >= split_waves"""
    sq = 0
    for q in range(1, {8: 4, 4: 3}.get(WK, 1)):
        if ntile * (WK >> q) >= split_waves:
            sq = q
    return WK >> sq


ALL_INSTANTIATIONS = sorted("sparse_conv_kernel<%d,%s,%s,%s,%s>" % (mr, taps, "true" if dual else "false", wkun, rows)
                            for taps, wkun, rows in (("9", "8,2", "true"), ("9", "8,2", "false"), ("1", "4,8", "false"))
                            for mr, dual in ((1, False), (2, False), (4, False), (1, True)))


# ---- the case table ------------------------------------------------------------------------------------------------------------------
DENSITIES = ("all", "30", "one", "17", "none")


def _case(key, kind, B, H, W, C1, up1, C2, Cout, ksize, want, **kw):
    c = dict(key=key, kind=kind, B=B, H=H, W=W, C1=C1, up1=up1, C2=C2, Cout=Cout, ksize=ksize, want=want, pads=("reflect",), act="elu", slope=0.0,
             out_scale=1.0, dual=False, C1tot=C1, c1_off=0, c1_off2=0, mask=ksize == 3, dens=DENSITIES, split_waves=0)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


_DUAL = dict(dual=True, act="sigmoid", out_scale=4.0, C1tot=48, c1_off2=24)
_K1 = dict(act="leaky", slope=0.1)
# `want` = (MR, TAPS, DUAL, ROWS) of the instantiation the row is there for; B, HxW, C1, up1, C2, Cout, k as the plan gives them, but for
# "k1_mr1": at 66x63 the host's rule already doubles MR for Cout = 19 (260 tiles x 2 out-channel tiles = 520 > 512), so the MR = 1
# row runs Cout = 19 on 30x63 (119 x 2 = 238)
TABLE = [
    _case("rows_w3", "y3", 1, 5, 3, 5, 1, 0, 4, 3, (1, 9, False, True), pads=("reflect", "zero")),               # the window is the whole row
    _case("rows_w1_3", "y3", 1, 6, 6, 6, 2, 3, 17, 3, (1, 9, False, True), pads=("reflect", "zero"), act="none"),  # W1 = 3; C1 = 6: a K-step's lanes read both sources
    _case("rows_mr2", "y3", 3, 40, 36, 7, 1, 0, 20, 3, (2, 9, False, True), pads=("zero", "reflect"), act="leaky", slope=0.1),   # 90 * 3 * 2 = 540 > 512
    _case("rows_mr4", "y3", 2, 38, 36, 9, 2, 6, 72, 3, (4, 9, False, True)),                                     # ncot = 5: 172 * 3 = 516 > 512 -> MR 4, 2 groups, 3 clamped tiles
    _case("narrow_w2", "y3", 1, 7, 2, 5, 1, 0, 4, 3, (1, 9, False, False), pads=("reflect", "zero")),
    _case("narrow_w1_2", "y3", 1, 6, 4, 4, 2, 3, 4, 3, (1, 9, False, False), pads=("reflect", "zero")),
    _case("narrow_mr2", "y3", 1, 1040, 4, 4, 2, 2, 32, 3, (2, 9, False, False), dens=("all", "30", "17")),           # 260 tiles
    _case("narrow_mr4", "y3", 1, 1040, 4, 4, 2, 2, 64, 3, (4, 9, False, False), pads=("zero",), dens=("all", "30", "17")),
    _case("k1_mr1", "y1", 1, 30, 63, 37, 1, 0, 19, 1, (1, 1, False, False), **_K1),
    _case("k1_mr2", "y1", 1, 66, 63, 37, 1, 0, 32, 1, (2, 1, False, False), **_K1),
    _case("k1_mr4", "y1", 1, 66, 63, 37, 1, 0, 40, 1, (4, 1, False, False), **_K1),                                # ncot 3 -> MR 4 with one clamped tile
    _case("dual_rows", "ydual", 1, 12, 10, 24, 1, 0, 3, 3, (1, 9, True, True), pads=("reflect", "zero"), **_DUAL),
    _case("dual_narrow", "ydual", 1, 12, 2, 24, 1, 0, 3, 3, (1, 9, True, False), pads=("reflect", "zero"), **_DUAL),
    _case("dual_k1", "ydual", 1, 12, 10, 24, 1, 0, 3, 1, (1, 1, True, False), **_DUAL),
    _case("dual_gap", "ydual", 1, 12, 10, 24, 1, 0, 3, 3, (1, 9, True, True), dens=("30",), dual=True, act="sigmoid", out_scale=4.0, C1tot=52, c1_off=1, c1_off2=27),
    _case("slice", "y3", 1, 8, 9, 5, 1, 0, 6, 3, (1, 9, False, True), C1tot=11, c1_off=3),                        # channels outside the slice are NaN
    _case("no_mask", "y3", 1, 8, 10, 5, 1, 0, 4, 3, (1, 9, False, True), mask=False, pads=("reflect", "zero")),
    _case("up2_no_x2", "y3", 1, 8, 10, 5, 2, 0, 4, 3, (1, 9, False, True)),
    # the device-side task loop: grid.x = 256 < 260 tiles at default settings (S = WK); 33 tasks of 8 tiles > grid.x = 32 at split_waves = 1
    _case("loop_default", "y3", 8, 66, 63, 4, 1, 0, 16, 3, (1, 9, False, True), dens=("all",)),
    _case("loop_s1", "y3", 64, 66, 63, 4, 1, 0, 16, 3, (1, 9, False, True), dens=("all",), split_waves=1),
]
CASES = {c["key"]: c for c in TABLE}
assert len(CASES) == len(TABLE)


def want_name(c):
    mr, taps, dual, rows = c["want"]
    return "sparse_conv_kernel<%d,%d,%s,%s,%s>" % (mr, taps, "true" if dual else "false", "8,2" if taps == 9 else "4,8", "true" if rows else "false")


def case_select(c, max_out=None, **switches):
    return select(c["B"], c["H"], c["W"], c["up1"], c["Cout"], c["ksize"], c["H"] * c["W"] if max_out is None else max_out, c["dual"], **switches)


def _gen(*tag):
    return torch.Generator().manual_seed(zlib.crc32(repr(tag).encode()))


def inputs(c):
    """The operands of a case (float32 / uint8, CPU, batched form), deterministic in the key.  Channels of x1 that no slice owns are NaN."""
    g = _gen("in", c["key"])
    B, H, W, C1, C2, Cout, k, up = c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"], c["ksize"], c["up1"]
    cin = C1 + C2
    x1 = torch.randn((B, c["C1tot"], H // up, W // up), generator=g)
    own = torch.zeros(c["C1tot"], dtype=torch.bool)
    own[c["c1_off"]:c["c1_off"] + C1] = True
    if c["dual"]:
        own[c["c1_off2"]:c["c1_off2"] + C1] = True
    x1[:, ~own] = NAN
    d = dict(x1=x1, x2=torch.randn((B, C2, H, W), generator=g) if C2 else None,
             in_mask=(torch.rand((B, H, W), generator=g) < 0.7).to(torch.uint8) if c["mask"] else None,
             w=torch.randn((Cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5, b=torch.randn(Cout, generator=g) * 0.1, w2=None, b2=None)
    if c["dual"]:
        d["w2"], d["b2"] = torch.randn((Cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5, torch.randn(Cout, generator=g) * 0.1
    return d


def out_mask(c, density):
    """[B,H,W] bool: the listed pixels of every frame at a density of the table"""
    g = _gen("out", c["key"], density)
    B, H, W = c["B"], c["H"], c["W"]
    if density == "all":
        return torch.ones((B, H, W), dtype=torch.bool)
    if density == "30":
        return torch.rand((B, H, W), generator=g) < 0.3
    m = torch.zeros((B, H * W), dtype=torch.bool)
    n = {"one": 1, "17": min(17, H * W), "none": 0}[density]    # 17: two tiles, the second with one live lane
    for f in range(B):
        m[f, torch.randperm(H * W, generator=g)[:n]] = True
    return m.view(B, H, W)


def raster_lists(om, max_out=None):
    """-> (coords [B,max_out] int32, counts [B]): raster order, for the oracle.  Entries past a frame's count are -1 and never go to
    the kernel: the GPU tests build their raster lists with the compaction kernel and compare its first `count` entries with these."""
    B = om.shape[0]
    npix = om[0].numel()
    max_out = npix if max_out is None else max_out
    coords = torch.full((B, max_out), -1, dtype=torch.int32)
    counts = []
    for f in range(B):
        idx = torch.nonzero(om[f].reshape(-1)).reshape(-1)
        coords[f, :min(idx.numel(), max_out)] = idx[:max_out].to(torch.int32)
        counts.append(int(idx.numel()))                                                   # may exceed max_out: the consumer clamps
    return coords, counts


def hand_lists(c, om, density):
    """-> (coords [B,H*W] int32, counts [B]): the listed pixels of every frame in a random order; the entries past the count are stale
    by contract and are filled with in-range indices of pixels that are NOT listed -- a kernel that used one would write there"""
    g = _gen("hand", c["key"], density)
    B, npix = om.shape[0], om[0].numel()
    coords = torch.zeros((B, npix), dtype=torch.int32)
    counts = []
    for f in range(B):
        flat = om[f].reshape(-1)
        idx, rest = torch.nonzero(flat).reshape(-1), torch.nonzero(~flat).reshape(-1)
        n = idx.numel()
        coords[f, :n] = idx[torch.randperm(n, generator=g)].to(torch.int32)
        if n < npix:
            coords[f, n:] = rest[torch.randperm(rest.numel(), generator=g)].to(torch.int32)     # exactly the npix - n unlisted pixels
        counts.append(int(n))
    return coords, counts


def oracle(c, d, coords, counts, max_out, pad, dtype):
    """the oracle on a case's operands `d` and pixel lists (batched form)"""
    return sparse_conv_oracle(d["x1"], d["w"], d["b"], coords, counts, max_out, c["H"], c["W"], c["ksize"], dtype, x2=d["x2"], up1=c["up1"],
                              in_mask=d["in_mask"], pad=pad, act=c["act"], slope=c["slope"], out_scale=c["out_scale"], c1=c["C1"], c1_off=c["c1_off"],
                              w2=d["w2"], b2=d["b2"], c1_off2=c["c1_off2"])


def poisoned(c, d):
    """A copy of the operands with NaN / +Inf / -Inf wherever the contract says nothing is read: x2 and x1 (up1 = 1) at every pixel
    where in_mask is 0; for up1 = 2 the coarse pixels of x1 whose four fine pixels are all masked.  (x1 channels that no slice owns
    are NaN in every run.)"""
    assert d["in_mask"] is not None
    bad = torch.tensor([NAN, float("inf"), -float("inf")])
    off = d["in_mask"] == 0                                                            # [B,H,W]
    q = dict(d)
    if d["x2"] is not None:
        x2 = d["x2"].clone()
        sel = off[:, None].expand_as(x2)
        x2[sel] = bad[torch.arange(int(sel.sum())) % 3]
        q["x2"] = x2
    off1 = off if c["up1"] == 1 else off.view(c["B"], c["H"] // 2, 2, c["W"] // 2, 2).all(4).all(2)
    x1 = d["x1"].clone()
    sel = off1[:, None].expand_as(x1)
    x1[sel] = bad[torch.arange(int(sel.sum())) % 3]
    q["x1"] = x1
    return q
