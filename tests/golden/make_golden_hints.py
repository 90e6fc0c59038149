"""Golden vectors for the depth-hint fusion, produced by the REFERENCE's own code.

KITTI/layers.py imports with torch and numpy only: its BackprojectDepth, Project3D and SSIM are used as they are.
KITTI/precompute_depth_hints.py cannot be imported (cv2, torchvision), so this script parses it, pulls
compute_reprojection_loss out with `ast` and executes exactly that definition against the reference's SSIM; the pieces are
then called in the order of `run` (lines 244-249) in float32 on the CPU, one image at a time with its M candidates as the
batch, as the script does.  The disparity conversion is line 149's expression.  Run in the build container only:

    python tests/golden/make_golden_hints.py        # writes tests/golden/hints_reference.npz

Per case of tests/hints_cases.py: the reference's best_index (uint8), its float32 losses and delta_ref = the largest
|reference float32 loss - float64 oracle loss| (tests/hints_ref.py).  Once: tol_loss = 2 max(delta_ref) -- a second float32
evaluation of the same formula (another summation order, fused multiply-adds) errs by the reference's own amount,
independently of it.  Nothing from /root/reference is stored, and no inputs: the tests regenerate them from
wavelet_monodepth_amd.synth.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/KITTI"
sys.path.insert(0, REF)
import hints_cases  # noqa: E402
import hints_ref  # noqa: E402
import layers as RL  # noqa: E402  (the reference's KITTI/layers.py)


def extract(path, names, namespace):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module([node], []), path, "exec"), namespace)
    missing = [n for n in names if n not in namespace]
    assert not missing, missing
    return namespace


def main():
    ns = extract(os.path.join(REF, "precompute_depth_hints.py"), ["compute_reprojection_loss"], {"torch": torch, "SSIM": RL.SSIM})
    reprojection_loss = ns["compute_reprojection_loss"]
    out, deltas = {}, []
    for name in hints_cases.CASES:
        case = hints_cases.build(name)
        B, M, H, W = case["cand"].shape
        cam_to_world, world_to_cam = RL.BackprojectDepth(M, H, W), RL.Project3D(M, H, W)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        index, losses = np.zeros((B, H, W), np.uint8), np.zeros((B, M, H, W), np.float32)
        for b in range(B):
            K, inv_K = t(case["K"][b])[None].expand(M, -1, -1), t(case["inv_K"][b])[None].expand(M, -1, -1)
            if case["disparities"]:
                disps = t(case["cand"][b])
                focal_baseline = K[0, 0, 0] * 0.1
                assert float(focal_baseline) == case["fbl"]
                depths = focal_baseline / (disps + 1e-7) * (disps > 0).float()          # line 149
                assert np.array_equal(depths.numpy().view(np.uint32), case["depths"][b].view(np.uint32))
            else:
                depths = t(case["cand"][b])
            base = t(case["base"][b])[None].expand(M, -1, -1, -1)
            lookup = t(case["lookup"][b])[None].expand(M, -1, -1, -1)
            with torch.no_grad():
                world_points = cam_to_world(depths, inv_K)                               # lines 244-248
                cam_pix = world_to_cam(world_points, K, t(case["T"][b])[None])
                sample = F.grid_sample(lookup, cam_pix, padding_mode="border")
                ls = reprojection_loss(sample, base)
                best_index = torch.argmin(ls, dim=0)
            index[b], losses[b] = best_index[0].numpy(), ls[:, 0].numpy()
        l64 = hints_ref.losses(case)
        delta = float(np.abs(losses.astype(np.float64) - l64).max())
        deltas.append(delta)
        out[name + "|index"], out[name + "|losses"], out[name + "|delta_ref"] = index, losses, np.array([delta])
    tol = 2.0 * max(deltas)
    out["tol_loss"] = np.array([tol])
    for name, delta in zip(hints_cases.CASES, deltas):
        case = hints_cases.build(name)
        dec = hints_ref.decisive(hints_ref.losses(case), case["depths"], tol)
        agree = hints_ref.gather(case["depths"], out[name + "|index"].astype(np.int64)) == \
            hints_ref.gather(case["depths"], hints_ref.first_argmin(hints_ref.losses(case)))
        print("%-20s delta_ref %.3e  decisive %.1f %%  reference depth == oracle depth at decisive pixels: %s, everywhere %.1f %%, "
              "no-match hints %.1f %%" % (name, delta, 100 * dec.mean(), bool(agree[dec].all()), 100 * agree.mean(),
                                          100 * (hints_ref.gather(case["depths"], out[name + "|index"].astype(np.int64)) == 0).mean()))
    print("tol_loss = %.3e" % tol)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "hints_reference.npz"), **out)


if __name__ == "__main__":
    main()
