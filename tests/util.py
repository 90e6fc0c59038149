"""Shared helpers for the test-suite (golden loading, deterministic inputs, comparisons)."""
import ast
import json
import os
import zlib

import numpy as np
import torch

from wavelet_monodepth_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
R18 = [64, 64, 128, 256, 512]
R50 = [64, 256, 512, 1024, 2048]


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def key_str(k):
    return k if isinstance(k, str) else "|".join(str(p) for p in k)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def sample(a, limit=4096):
    flat = np.asarray(a).reshape(-1)
    step = max(1, -(-flat.size // limit))
    return flat[::step]


def kitti_feats(batch, h, w, chans=R18, seed=1):
    return [t(f) for f in synth.encoder_features(batch, h, w, chans, seed=seed)]


def nyu_feats(batch, h, w, enc, seed=8, prefix="nyu_feat"):
    return [t(synth.normal((batch, c, h >> (k + 1), w >> (k + 1)), "%s%d" % (prefix, k), seed)) for k, c in enumerate(enc)]


def max_rel(a, b):
    """max |a-b| / max(|b|, 1e-6 * max|b|) -> a robust scalar relative error"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1e-30)
    return float(np.abs(a - b).max() / scale)


def assert_close(a, b, rtol, what=""):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    err = max_rel(a, b)
    assert err <= rtol, "%s: max relative error %.3e > %.1e" % (what, err, rtol)


def assert_depth_close(disp_got, disp_ref, rtol, what="", min_depth=0.1, max_depth=100.0):
    """north_star's tolerance is "<= 1e-4 relative on depth maps": checked PER PIXEL on depth = 1 / (min_disp + (max_disp -
    min_disp) * disp) (KITTI/layers.py:16-25), where a norm-wise bound on the disparity is blind at small disparities."""
    to = lambda v: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float64)
    lo, hi = 1.0 / max_depth, 1.0 / min_depth
    dg, dr = 1.0 / (lo + (hi - lo) * to(disp_got)), 1.0 / (lo + (hi - lo) * to(disp_ref))
    rel = float((np.abs(dg - dr) / np.abs(dr)).max())
    assert rel <= rtol, "%s: per-pixel relative depth error %.3e > %.1e" % (what, rel, rtol)


def photo_case(B=2, H=24, W=40, seed=31):
    """Two frames, a depth map, KITTI-like intrinsics and a small rigid motion — shared with the tests."""
    tgt = synth.uniform((B, 3, H, W), "ph_tgt", seed, 0.0, 1.0).astype(np.float32)
    src = synth.uniform((B, 3, H, W), "ph_src", seed, 0.0, 1.0).astype(np.float32)
    # smooth the frames a little so the bilinear sampling gradient is informative
    k = np.ones((3, 3), np.float32) / 9
    for a in (tgt, src):
        pad = np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
        a[:] = sum(pad[:, :, i:i + H, j:j + W] * k[i, j] for i in range(3) for j in range(3))
    depth = synth.uniform((B, 1, H, W), "ph_depth", seed, 2.0, 30.0).astype(np.float32)
    K = np.tile(np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32), (B, 1, 1))
    inv_K = np.linalg.inv(K).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    for b in range(B):
        ang = 0.02 * (b + 1)
        T[b, :3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
        T[b, :3, 3] = [0.3 * (b + 1), -0.05, 0.4]
    return tgt, src, depth, K, inv_K, T


def loss_case(B=2, H=32, W=64, seed=17, hints=False):
    """A synthetic minibatch for the photometric loss: colour pyramids of frames 0, -1, 1 (and "s"), intrinsics, poses,
    4 disparity scales.  -> (inputs, outputs) dicts of numpy arrays keyed like the reference trainer's."""
    from wavelet_monodepth_amd import synth
    frame_ids = [0, -1, 1] + (["s"] if hints else [])
    inputs, outputs = {}, {}
    k3 = np.ones((3, 3), np.float32) / 9
    for f in frame_ids:
        img = synth.uniform((B, 3, H, W), "lc_img%s" % f, seed, 0.0, 1.0).astype(np.float32)
        pad = np.pad(img, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
        img = sum(pad[:, :, i:i + H, j:j + W] * k3[i, j] for i in range(3) for j in range(3)).astype(np.float32)
        for s in range(4):
            h, w = H >> s, W >> s
            inputs[("color", f, s)] = img.reshape(B, 3, h, 1 << s, w, 1 << s).mean((3, 5)).astype(np.float32)
    K = np.tile(np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32), (B, 1, 1))
    inputs[("K", 0)], inputs[("inv_K", 0)] = K, np.linalg.inv(K).astype(np.float32)
    for f, tx in ((-1, -0.2), (1, 0.25)):
        T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
        T[:, 0, 3], T[:, 2, 3] = tx, 0.1 * tx
        outputs[("cam_T_cam", 0, f)] = T
    st = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    st[:, 0, 3] = 0.1
    inputs["stereo_T"] = st
    for s in range(4):
        outputs[("disp", s)] = synth.uniform((B, 1, H >> s, W >> s), "lc_disp%d" % s, seed, 0.05, 0.9).astype(np.float32)
    if hints:
        inputs["depth_hint"] = synth.uniform((B, 1, H, W), "lc_hint", seed, 1.0, 40.0).astype(np.float32)
        inputs["depth_hint_mask"] = (synth.uniform((B, 1, H, W), "lc_hmask", seed, 0.0, 1.0) > 0.3).astype(np.float32)
    return inputs, outputs


def scaled_intrinsics(B, H, W):
    """KITTI-like K and inv_K [B,4,4] for an H x W frame (the intrinsics of photo_case)"""
    K = np.tile(np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32), (B, 1, 1))
    return K, np.linalg.inv(K).astype(np.float32)


def box3(a):
    """3x3 box blur with edge padding, in place (the smoothing of photo_case)."""
    H, W = a.shape[-2:]
    pad = np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
    a[:] = sum(pad[:, :, i:i + H, j:j + W] for i in range(3) for j in range(3)) / np.float32(9)
    return a


WARP_MARGIN = 1e-3   # px: a sample this close to an integer or to a clamp edge is excluded from the gradient comparison


def warp_edge_case(B, C, H, W, Hs, Ws, seed):
    """Inputs of warp_frame for a [B,C,Hs,Ws] source sampled into a [B,1,H,W] target: intrinsics scaled to the target size, a
    small pose (a yaw of 0.02 (b+1) rad, a translation of (0.3 (b+1), -0.05, -0.2): the camera backs off, so samples leave
    over all four borders), depths in 2-30 (uniform in the disparity, like a street scene).  Also the float64 sample
    coordinates (ux, uy) [B,H,W] in source pixels, and `excl` [B,H,W]: ux or uy within WARP_MARGIN of an integer (the bilinear
    cell changes there and d out / d coord jumps) or of a clamp edge 0 / size-1 (the clip multiplier jumps between 0 and 1).
    `gout` [B,C,H,W] is the upstream gradient, zero at excluded pixels, so that neither ddepth there nor the dT sum depends
    on which side of the jump a rounding lands.  `clamped` is the share of the 2*B*H*W coordinates on the border clamp."""
    src = box3(synth.uniform((B, C, Hs, Ws), "we_src", seed, 0.0, 1.0).astype(np.float32))
    disp = synth.uniform((B, 1, H, W), "we_disp", seed, 1.0 / 30.0, 0.5).astype(np.float32)
    depth = np.clip(1.0 / disp.astype(np.float64), 2.0, 30.0).astype(np.float32)
    K, inv_K = scaled_intrinsics(B, H, W)
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    for b in range(B):
        ang = 0.02 * (b + 1)
        T[b, :3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
        T[b, :3, 3] = [0.3 * (b + 1), -0.05, -0.2]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([xs.reshape(-1), ys.reshape(-1), np.ones(H * W)], 0)
    cam = depth.astype(np.float64).reshape(B, 1, -1) * (inv_K.astype(np.float64)[:, :3, :3] @ pix)
    cam = np.concatenate([cam, np.ones((B, 1, H * W))], 1)
    c = (K.astype(np.float64) @ T.astype(np.float64))[:, :3, :] @ cam
    ux = (c[:, 0] / (c[:, 2] + 1e-7)).reshape(B, H, W) * Ws / (W - 1) - 0.5
    uy = (c[:, 1] / (c[:, 2] + 1e-7)).reshape(B, H, W) * Hs / (H - 1) - 0.5
    near = lambda u: np.abs(u - np.rint(u)) < WARP_MARGIN      # the clamp edges 0 and size-1 are integers themselves
    excl = near(ux) | near(uy)
    clamped = lambda u, n: (u <= 0) | (u >= n - 1)
    gout = synth.uniform((B, C, H, W), "we_g", seed, 0.0, 1.0).astype(np.float32) * ~excl[:, None]
    return dict(src=src, depth=depth, K=K, inv_K=inv_K, T=T, ux=ux, uy=uy, excl=excl, gout=gout,
                clamped=float((clamped(ux, Ws).mean() + clamped(uy, Hs).mean()) / 2))


def smooth_tie_case(B, C, H, W, seed):
    """disp [B,1,H,W] in 0.05-0.9 and img [B,C,H,W] for get_smooth_loss, with the two places where |a - b| is delicate:
    constant 3x3 patches (clipped to H x (W-1) on tiny maps, so that the map never goes constant), whose inner pairs are
    exact ties (sgn(0) == 0: no gradient from either side), and neighbours one ulp apart (the sign must survive)."""
    disp = synth.uniform((B, 1, H, W), "st_disp", seed, 0.05, 0.9).astype(np.float32)
    img = synth.uniform((B, C, H, W), "st_img", seed, 0.0, 1.0).astype(np.float32)
    g = np.random.default_rng(zlib.crc32(b"smooth_tie") + seed)
    ph, pw = min(3, H), min(3, W - 1)
    n = max(1, B * H * W // 128)
    for b, y, x in zip(g.integers(0, B, n), g.integers(0, H - ph + 1, n), g.integers(0, W - pw + 1, n)):
        disp[b, 0, y:y + ph, x:x + pw] = disp[b, 0, y, x]
    for b, y, x in zip(g.integers(0, B, n), g.integers(0, H, n), g.integers(0, W - 1, n)):
        disp[b, 0, y, x + 1] = np.nextafter(disp[b, 0, y, x], np.float32(1 if (x + y) & 1 else 0))
    return disp, img


def fully_tied(disp):
    """[B,1,H,W] mask of the pixels all of whose neighbour pairs (left, right, up, down, where they exist) are exact ties"""
    d = disp[:, 0]
    m = np.ones(d.shape, bool)
    ex, ey = d[:, :, :-1] == d[:, :, 1:], d[:, :-1, :] == d[:, 1:, :]
    m[:, :, :-1] &= ex
    m[:, :, 1:] &= ex
    m[:, :-1, :] &= ey
    m[:, 1:, :] &= ey
    return m[:, None]


SSIM_L1_MARGIN = 1e-6   # |x - y| below this: d|x - y| jumps; excluded from the gradient comparison


def ssim_edge_case(B, C, H, W, seed, smoothed):
    """Two frames in [0, 1) for SSIM / compute_reprojection_loss: 3x3-smoothed (E[x^2] - mu^2 cancels: the hard numerical
    case) or iid (where L1 ties essentially cannot occur); upstream gradients `w` [B,C,H,W] (mode 0) and `w1` [B,1,H,W]
    (mode 1); `excl` [B,C,H,W] marks |x - y| < SSIM_L1_MARGIN."""
    x = synth.uniform((B, C, H, W), "se_x", seed, 0.0, 1.0).astype(np.float32)
    y = synth.uniform((B, C, H, W), "se_y", seed, 0.0, 1.0).astype(np.float32)
    if smoothed:
        box3(x), box3(y)
    w = synth.uniform((B, C, H, W), "se_w", seed, 0.0, 1.0).astype(np.float32)
    w1 = synth.uniform((B, 1, H, W), "se_w1", seed, 0.0, 1.0).astype(np.float32)
    excl = np.abs(x.astype(np.float64) - y.astype(np.float64)) < SSIM_L1_MARGIN
    return dict(x=x, y=y, w=w, w1=w1, excl=excl)


# ---- the photometric oracle (oracle/photo_ref.py) at a chosen precision; every result comes back as float64 numpy -------

def _td(a, dtype, g=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(g)


def _n64(v):
    return v.detach().double().numpy()


def oracle_warp(case, dtype):
    """-> (out, ddepth, dT) of oracle.photo_ref.warp_frame with the upstream gradient case["gout"]"""
    from oracle import photo_ref as P
    d, T = _td(case["depth"], dtype, True), _td(case["T"], dtype, True)
    out = P.warp_frame(_td(case["src"], dtype), d, _td(case["K"], dtype), _td(case["inv_K"], dtype), T)
    (out * _td(case["gout"], dtype)).sum().backward()
    return _n64(out), _n64(d.grad), _n64(T.grad)


def oracle_ssim(case, mode, dtype):
    """mode "ssim": the SSIM module; "reproj" / "l1": compute_reprojection_loss with / without SSIM -> (out, dx, dy)"""
    from oracle import photo_ref as P
    x, y = _td(case["x"], dtype, True), _td(case["y"], dtype, True)
    out = P.ssim(x, y) if mode == "ssim" else P.compute_reprojection_loss(x, y, mode == "reproj")
    (out * _td(case["w" if mode == "ssim" else "w1"], dtype)).sum().backward()
    return _n64(out), _n64(x.grad), _n64(y.grad)


SMOOTH_UPSTREAM = 0.37   # d(loss)/d(smoothness) handed to the backward: not 1, so that a dropped factor shows


def oracle_smooth(disp, img, dtype):
    """-> (value, ddisp) of get_smooth_loss, backward from SMOOTH_UPSTREAM * value"""
    from oracle import photo_ref as P
    d = _td(disp, dtype, True)
    sm = P.get_smooth_loss(d, _td(img, dtype))
    (sm * SMOOTH_UPSTREAM).backward()
    return _n64(sm), _n64(d.grad)


def edge_err(a, ref64, keep=None):
    """max |a - ref64| over the kept entries, relative to max |ref64| (absolute where the reference is all zero)"""
    a, ref64 = np.asarray(a, np.float64), np.asarray(ref64, np.float64)
    diff = np.abs(a - ref64)
    if keep is not None:
        diff = diff[np.broadcast_to(keep, diff.shape)]
    scale = float(np.abs(ref64).max()) if ref64.size else 0.0
    return float(diff.max()) / (scale if scale > 0 else 1.0) if diff.size else 0.0


# (B, C, H, W, Hs, Ws) of tests/test_gpu_photo_edges.py: general shapes, source sizes, then the reduce edges of
# warp_bwd_kernel -> warp_bwd_finish_kernel (nblk = ceil(H W / 1024) capped at 256)
WARP_CASES = [(2, 3, 5, 7, 5, 7), (3, 1, 17, 33, 17, 33), (2, 3, 16, 24, 8, 12), (2, 3, 12, 20, 24, 40),
              (1, 3, 32, 32, 32, 32), (2, 3, 25, 41, 25, 41), (1, 3, 256, 256, 256, 256), (1, 3, 257, 256, 257, 256),
              (1, 3, 513, 512, 513, 512)]
WARP_DEGENERATE = [(1, 3, 2, 2, 2, 2), (1, 3, 16, 24, 1, 1)]
# (B, C, H, W): nblk = ceil(B H W / 2048) capped at 512
SMOOTH_CASES = [(1, 1, 2, 2), (2, 3, 5, 7), (1, 3, 32, 64), (1, 3, 3, 683), (1, 3, 257, 512), (1, 1, 1025, 1024)]
SSIM_SMALL = [(1, 3, 2, 2), (1, 1, 2, 9), (2, 3, 3, 2), (2, 3, 5, 7), (1, 3, 17, 33)]
SSIM_WRAP = [((1, 3, 700, 1000), "ssim"), ((1, 1, 1025, 2050), "reproj")]   # n > 8192 * 256: the grid-stride loop runs twice


def check_packed(out, gold, tol, exact=True, limit=4096):
    """Compare a decoder output dict with a PACKED full-size fixture (tests/golden/make_golden.py::pack_outputs): float
    maps as strided samples ("s|key"), boolean masks bit-packed ("m|key" + "mshape|key"), integers ("i|key")."""
    want = {k.split("|", 1)[1] for k in gold if k[:2] in ("s|", "m|", "i|")}
    have = {key_str(k) for k in out}
    assert want == have, want ^ have
    for k, v in out.items():
        ks = key_str(k)
        if torch.is_tensor(v) and v.dtype.is_floating_point:
            assert_close(sample(v.detach().cpu().numpy(), limit), gold["s|" + ks], tol, ks)
        elif torch.is_tensor(v):
            shape = tuple(int(n) for n in gold["mshape|" + ks])
            ref = np.unpackbits(gold["m|" + ks])[:int(np.prod(shape))].reshape(shape)
            assert tuple(v.shape) == shape, ks
            if exact:
                assert np.array_equal(v.cpu().numpy().astype(np.uint8), ref), ks
        elif exact:
            assert int(v) == int(gold["i|" + ks]), "%s: %d vs %d" % (ks, int(v), int(gold["i|" + ks]))


def unpack_mask(gold, key):
    shape = tuple(int(n) for n in gold["mshape|" + key])
    return np.unpackbits(gold["m|" + key])[:int(np.prod(shape))].reshape(shape)


def quarter_family_declines(name, C1, C2, masked=False, up=1, promise=1):
    """conv_wino32q_kernel (round 5) takes pure layers only -- every 8-channel chunk inside one source tensor, and an input mask
    over an upsampled operand only under the 2x2-constant promise (it has no generic gather); a forced launch on anything else
    must return WMD_ERR_UNSUPPORTED (-3) instead of computing something."""
    if not name.startswith("conv_wino32q"):
        return False
    return (C1 + C2) % 8 != 0 or (C2 > 0 and C1 % 8 != 0) or (masked and up == 2 and not promise)


def family(name):
    if name.startswith("conv_wino32q"):
        return "wino32q"
    if name.startswith("conv_wino32"):
        return "wino32"
    if name.startswith("conv_wino"):
        return "wino"
    return "1x1" if name.endswith(",1>") else "direct3x3"


def serves(name, k):
    """the tuner's candidate filter (tuner.tune): direct kernels of the layer's tap count, every Winograd entry for 3x3"""
    return name.endswith(",%d>" % (9 if k == 3 else 1)) or (k == 3 and name.startswith("conv_wino"))


def chunk_channels(name):
    """CK of a table entry: the last template argument of the Winograd kernels, the one before TAPS of conv_fwd_kernel"""
    args = name[name.index("<") + 1:-1].split(",")
    return int(args[-1] if name.startswith("conv_wino") else args[-2])


def split_accepted(name, ks, red):
    """Must the planner accept a forced split ks of a reduction over `red` channels?  k > 0 needs k chunks; -k (the second-stage
    sum of a kernel that also finishes in-kernel) exists for the 32x32x2 families only."""
    nchunks = -(-red // chunk_channels(name))
    if ks < 0 and not family(name).startswith("wino32"):
        return False
    return nchunks >= abs(ks)


def offered_splits():
    """the tuner's whole offer (tuner.tune): k slices (finished in-kernel by the 32x32x2 families, by the second-stage kernel
    elsewhere) and -k (the second-stage form of a kernel that has both; the planner must refuse it for the others)"""
    from wavelet_monodepth_amd import tuner
    return tuple(tuner.KSPLITS) + tuple(-k for k in tuner.KSPLITS if k > 1)


def bench_tune_cache_name():
    """bench.TUNE_CACHE, read without executing bench.py (collection must not start anything); the tests check it against the
    imported module"""
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t_, "id", None) == "TUNE_CACHE" for t_ in node.targets):
            return node.value.value
    raise AssertionError("bench.py has no TUNE_CACHE")


def committed_entries():
    """the tile choices bench.py preloads: sorted (key, (label, split)) pairs"""
    with open(os.path.join(ROOT, "profiles", bench_tune_cache_name())) as f:
        return sorted((k, tuple(v)) for k, v in json.load(f).items())


def channel_subset(n, tag):
    """A deterministic subset of n channels: the first and last, both sides of the first two and the last 8 / 16 / 32-channel
    boundaries, and six at random (fixed seed)."""
    s = {0, n - 1}
    for q in (8, 16, 32):
        for b in (q, 2 * q, ((n - 1) // q) * q):
            if 0 < b < n:
                s.update((b - 1, b))
    g = np.random.default_rng(zlib.crc32(tag.encode()))
    s.update(int(v) for v in g.integers(0, n, 6))
    return sorted(s)
