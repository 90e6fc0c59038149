"""Inputs of the depth-hint tests, regenerated from wavelet_monodepth_amd.synth (numpy only, no transcendental functions):
the fixture tests/golden/hints_reference.npz stores the expected outputs of every case below, the tests rebuild the inputs.

A case is a dict of float32 arrays:
    cand [B,M,H,W]    what the caller hands over: pixel disparities (multiples of 1/4 around a smooth field, like a block
                      matcher's fixed-point output), or -- `disparities` False -- the depths themselves
    depths [B,M,H,W]  the candidates as depths: focal * baseline / (d + 1e-7) * (d > 0) in float32
    base, lookup [B,3,H,W] in [0,1]: a textured image, and the same image moved by a few pixels plus noise
    K, inv_K [B,4,4]  the reference's intrinsics (0.58 W, 1.92 H); T [B,4,4] the identity with T[0,3] = -0.1 for even b (a
                      left base image) and +0.1 for odd b, so one batch holds both signs
About 15 % of every candidate map is 0 ("no match"); candidate 1 is a copy of candidate 0 (exact ties) when M >= 2; in maps
of at least 12 x 12 a 5 x 6 block has every candidate 0 (`zero_block`: (y0, y1, x0, x1), the same in every image): the hint
is 0 on the whole block, and inside its one-pixel rim, where every candidate's 3 x 3 window is the same, index 0 wins.
"""
import numpy as np

from util import box3
from wavelet_monodepth_amd import synth

BASELINE = np.float32(0.1)

# name -> (B, M, H, W, given as disparities)
CASES = {
    "b1_m12_13x21": (1, 12, 13, 21, True),
    "b2_m5_33x70": (2, 5, 33, 70, True),
    "b3_m1_2x2": (3, 1, 2, 2, True),             # the smallest legal map, one candidate
    "b1_m12_64x96": (1, 12, 64, 96, True),       # whole 64 x 8 tiles and a half-filled one to their right
    "b2_m3_17x131": (2, 3, 17, 131, True),       # three tiles across and down, the last ragged in both directions
    "depths_b2_m4_24x40": (2, 4, 24, 40, False),
}
SHARE_CASES = tuple(n for n, (B, M, H, W, _) in CASES.items() if H * W >= 256)   # the decisive share is asserted here


def triangle(t, period):
    """a triangle wave of t in 0..1 (exact float arithmetic)"""
    return np.abs((t % period) / period - 0.5) * 2.0


def texture(B, H, W, tag):
    """[B,3,H,W] float64 in [0,1]: smoothed noise over slanted stripes of a few pixels' period"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    noise = box3(synth.uniform((B, 3, H, W), tag + "_tex", 5, 0.0, 1.0).astype(np.float64))
    img = np.empty((B, 3, H, W))
    for b in range(B):
        for c in range(3):
            stripes = triangle(xs * (1.0 + 0.25 * c) + ys * (0.5 + 0.125 * b), 7.0 + 2.0 * c)
            img[b, c] = 0.6 * noise[b, c] + 0.4 * stripes
    return np.clip(img, 0.0, 1.0)


def disparity_to_depth(d, fbl):
    """precompute_depth_hints.py:149 in float32 numpy"""
    d = d.astype(np.float32)
    return (np.float32(fbl) / (d + np.float32(1e-7)) * (d > 0).astype(np.float32)).astype(np.float32)


def build(name):
    B, M, H, W, as_disp = CASES[name]
    K = np.tile(np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32), (B, 1, 1))
    fx, fy, cx, cy = (float(v) for v in (K[0, 0, 0], K[0, 1, 1], K[0, 0, 2], K[0, 1, 2]))
    inv_K = np.tile(np.array([[1 / fx, 0, -cx / fx, 0], [0, 1 / fy, -cy / fy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32), (B, 1, 1))
    sign = np.array([-1.0 if b % 2 == 0 else 1.0 for b in range(B)])
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, 0, 3] = (sign * 0.1).astype(np.float32)
    fbl = float(K[0, 0, 0] * BASELINE)                     # a float32 product

    base = texture(B, H, W, name)
    shift = 2 if W < 40 else 3
    noise = synth.uniform((B, 3, H, W), name + "_noise", 6, -0.02, 0.02).astype(np.float64)
    # a candidate of disparity d samples the lookup image near x + sign * d: the lookup image is the base moved that way
    lookup = np.stack([np.roll(base[b], int(sign[b]) * shift, axis=-1) for b in range(B)])
    lookup = np.clip(lookup + noise, 0.0, 1.0)

    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64) / H, np.arange(W, dtype=np.float64) / W, indexing="ij")
    field = shift + 0.5 * (triangle(xs + 0.5 * ys, 0.75) - 0.5)
    step = 0.25 if W < 40 else 0.5
    wob = synth.uniform((B, M, H, W), name + "_wob", 7, -0.25, 0.25).astype(np.float64)
    off = np.array([((m * 5) % M - (M - 1) / 2.0) * step for m in range(M)])
    disp = np.maximum(np.round((field[None, None] + off[None, :, None, None] + wob) * 4.0) / 4.0, 0.5)
    disp[synth.uniform((B, M, H, W), name + "_miss", 8, 0.0, 1.0) < 0.15] = 0.0
    if M >= 2:
        disp[:, 1] = disp[:, 0]
    zero_block = None
    if H >= 12 and W >= 12:
        zero_block = (H // 2, H // 2 + 5, W // 3, W // 3 + 6)
        disp[:, :, zero_block[0]:zero_block[1], zero_block[2]:zero_block[3]] = 0.0
    disp = disp.astype(np.float32)
    depths = disparity_to_depth(disp, fbl)
    return dict(cand=disp if as_disp else depths, disparities=as_disp, fbl=fbl, depths=depths, base=base.astype(np.float32),
                lookup=lookup.astype(np.float32), K=K, inv_K=inv_K, T=T, zero_block=zero_block, duplicate=M >= 2)
