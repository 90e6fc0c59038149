"""Time the pose path, forward + backward, against the same arithmetic written with stock torch ops on the same GPU:

  the pose tail   ops.pose_head (1x1 + mean + scale + split + transforms: 1 launch forward, 2 backward) at [12,256,6,20] with
                  F = 1 and F = 2 and at [8,256,10,32] with F = 2, against conv2d -> mean -> scale -> slices ->
                  rot_from_axisangle / get_translation_matrix / matmul as elementwise and indexed-assignment launches
  PoseDecoder     the whole decoder at ResNet18 / 640x192 / batch 12 (last map [12,512,6,20]): one feature and two frames (the
                  separate_resnet form) and two features and one frame (the shared form), against torch.nn.functional convolutions
                  + the stock tail

Each is timed eagerly (host clock around `--iters` steps that end in a device synchronise) and as a hipGraph replay, fused and
stock alternating within every round; the figure is the median over `--rounds` rounds, with the spread (min - max) beside it.
Prints a markdown table (profiles/pose_path.md keeps one).

    python tools/pose_microbench.py [--iters 200] [--rounds 7] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from wavelet_monodepth_amd import ops, synth  # noqa: E402
from wavelet_monodepth_amd.kitti import PoseDecoder  # noqa: E402


def stock_rotation(vec):
    """axis-angle [B,1,3] -> [B,4,4] the way stock tensor code writes it: a zero matrix filled entry by entry"""
    angle = torch.norm(vec, 2, 2, True)
    axis = vec / (angle + 1e-7)
    ca, sa = torch.cos(angle), torch.sin(angle)
    C = 1 - ca
    x, y, z = (axis[..., k].unsqueeze(1) for k in range(3))
    rot = torch.zeros((vec.shape[0], 4, 4), device=vec.device)
    entries = {(0, 0): x * x * C + ca, (0, 1): x * y * C - z * sa, (0, 2): z * x * C + y * sa,
               (1, 0): x * y * C + z * sa, (1, 1): y * y * C + ca, (1, 2): y * z * C - x * sa,
               (2, 0): z * x * C - y * sa, (2, 1): y * z * C + x * sa, (2, 2): z * z * C + ca}
    for (i, j), v in entries.items():
        rot[:, i, j] = torch.squeeze(v)
    rot[:, 3, 3] = 1
    return rot


def stock_transform(axisangle, translation, invert):
    R = stock_rotation(axisangle)
    t = translation.clone()
    if invert:
        R = R.transpose(1, 2)
        t = t * -1
    T = torch.zeros(t.shape[0], 4, 4, device=t.device)
    for k in range(4):
        T[:, k, k] = 1
    T[:, :3, 3, None] = t.contiguous().view(-1, 3, 1)
    return torch.matmul(R, T) if invert else torch.matmul(T, R)


def stock_tail(x, w, b, frames, invert_mask):
    out = 0.01 * F.conv2d(x, w, b).mean(3).mean(2).view(-1, frames, 1, 6)
    aa, tr = out[..., :3], out[..., 3:]
    T = torch.stack([stock_transform(aa[:, f], tr[:, f], bool(invert_mask >> f & 1)) for f in range(frames)], 1)
    return aa, tr, T


def stock_decoder(module, feats, invert_mask):
    sq, p0, p1, p2 = module.net
    x = torch.cat([F.relu(F.conv2d(f, sq.weight, sq.bias)) for f in feats], 1)
    x = F.relu(F.conv2d(x, p0.weight, p0.bias, padding=1))
    x = F.relu(F.conv2d(x, p1.weight, p1.bias, padding=1))
    return stock_tail(x, p2.weight, p2.bias, module.num_frames_to_predict_for, invert_mask)


def make_step(forward, leaves, grads):
    def step():
        outs = forward()
        loss = sum((o * g).sum() for o, g in zip(outs, grads))
        return torch.autograd.grad(loss, leaves)
    return step


def time_loop(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = step()
    return g, keep


def bench(name, fused, stock, iters, rounds):
    """-> one table row: medians (and spread) of fused / stock, eager and replayed, in microseconds per step"""
    for _ in range(5):
        fused()
        stock()
    gf, kf = capture(fused)
    gs, ks = capture(stock)
    cols = {"eager fused": [], "eager stock": [], "graph fused": [], "graph stock": []}
    for _ in range(rounds):
        cols["eager fused"].append(time_loop(fused, iters))
        cols["eager stock"].append(time_loop(stock, iters))
        cols["graph fused"].append(time_loop(gf.replay, iters))
        cols["graph stock"].append(time_loop(gs.replay, iters))
    cell = lambda v: "%.1f (%.1f - %.1f)" % (statistics.median(v), min(v), max(v))
    med = {k: statistics.median(v) for k, v in cols.items()}
    return "| %s | %s | %s | %.2f | %s | %s | %.2f |" % (name, cell(cols["eager fused"]), cell(cols["eager stock"]),
                                                        med["eager stock"] / med["eager fused"], cell(cols["graph fused"]),
                                                        cell(cols["graph stock"]), med["graph stock"] / med["graph fused"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pose_microbench measures on the GPU only"
    dev = torch.device("cuda:0")
    t = lambda a, g=False: torch.from_numpy(a).to(dev).requires_grad_(g)
    rows = ["| case | eager fused us | eager stock us | stock / fused | graph fused us | graph stock us | stock / fused |",
            "|---|---|---|---|---|---|---|"]
    for (B, C, H, W), frames in (((12, 256, 6, 20), 1), ((12, 256, 6, 20), 2), ((8, 256, 10, 32), 2)):
        x = t(synth.normal((B, C, H, W), "mb_x", 1), True)
        w = t(synth.uniform((6 * frames, C, 1, 1), "mb_w", 1, -1 / 16, 1 / 16), True)
        b = t(synth.uniform((6 * frames,), "mb_b", 1, -1 / 16, 1 / 16), True)
        grads = [t(synth.uniform(s, "mb_g%d" % i, 1)) for i, s in enumerate(((B, frames, 1, 3), (B, frames, 1, 3), (B, frames, 4, 4)))]
        fused = make_step(lambda: ops.pose_head(x, w, b, frames, invert_mask=1), [x, w, b], grads)
        stock = make_step(lambda: stock_tail(x, w, b, frames, 1), [x, w, b], grads)
        rows.append(bench("tail [%d,%d,%d,%d] F=%d" % (B, C, H, W, frames), fused, stock, args.iters, args.rounds))
    for label, nfeat, frames in (("one feature, two frames", 1, 2), ("two features, one frame", 2, 1)):
        module = synth.fill_state_dict(PoseDecoder(np.array([64, 64, 128, 256, 512]), nfeat, frames), seed=1).to(dev)
        feats = [t(np.maximum(synth.normal((12, 512, 6, 20), "mb_f%d" % i, 1), 0.0), True) for i in range(nfeat)]
        grads = [t(synth.uniform(s, "mb_dg%d" % i, 1)) for i, s in enumerate(((12, frames, 1, 3), (12, frames, 1, 3), (12, frames, 4, 4)))]
        leaves = feats + list(module.parameters())
        fused = make_step(lambda: module.forward_transforms([[f] for f in feats], invert_mask=1), leaves, grads)
        stock = make_step(lambda: stock_decoder(module, feats, 1), leaves, grads)
        rows.append(bench("PoseDecoder R18 640x192 b12, %s" % label, fused, stock, args.iters, args.rounds))
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
