"""Golden vectors for the pose path from the REFERENCE's own classes: transformation_from_parameters (KITTI/layers.py),
PoseDecoder and PoseCNN -- outputs and gradients on the seeded inputs of tests/pose_cases.py, in float32 and in float64
(the reference builds its matrices with torch.zeros and no dtype, so the float64 run sets the default dtype) -- and the
state_dict manifests (names and shapes) of both classes.  Run in the build container only, with the reference on the path:

    PYTHONPATH=tests/golden/refshim:/root/reference/KITTI python tests/golden/make_golden_pose.py

writes tests/golden/kitti_pose.npz and tests/golden/state_dict_manifest_pose.json.  Large gradients are stored as
util.sample strides (pose_cases.SAMPLE entries)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from wavelet_monodepth_amd import synth  # noqa: E402
import pose_cases as PC  # noqa: E402
from util import sample  # noqa: E402
from networks.decoders.pose_decoder import PoseDecoder  # noqa: E402  (the reference's)
from networks.pose_cnn import PoseCNN  # noqa: E402
import layers as RL  # noqa: E402  (the reference's KITTI/layers.py)

DTYPES = {"f32": torch.float32, "f64": torch.float64}


def build(kind, kw):
    if kind == "cnn":
        return PoseCNN(**kw)
    return PoseDecoder(np.array(kw["num_ch_enc"]), **{k: v for k, v in kw.items() if k != "num_ch_enc"})


def main():
    out = {}
    for tag, dtype in DTYPES.items():
        torch.set_default_dtype(dtype)
        v, t, g = PC.transform_case(PC.TRANSFORM_N)
        for invert in (False, True):
            vv, tt = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (v, t))
            T = RL.transformation_from_parameters(vv[:, None], tt[:, None], invert)
            assert T.dtype == dtype
            (T * torch.from_numpy(g).to(dtype)).sum().backward()
            pre = "tf|%s|inv%d|" % (tag, invert)
            out[pre + "T"], out[pre + "dv"], out[pre + "dt"] = T.detach().numpy(), vv.grad.numpy(), tt.grad.numpy()
        for name, (kind, kw, _) in PC.NETS.items():
            m = synth.fill_state_dict(build(kind, kw), seed=PC.SEED).to(dtype)
            for k, a in PC.run_net(m, name, dtype).items():
                out["%s|%s|%s" % (name, tag, k)] = a if k in ("axisangle", "translation") else sample(a, PC.SAMPLE)
                if tag == "f32":
                    out["%s|%s|%s" % (name, tag, k)] = out["%s|%s|%s" % (name, tag, k)].astype(np.float32)
    torch.set_default_dtype(torch.float32)
    np.savez_compressed(os.path.join(HERE, "kitti_pose.npz"), **out)
    manifest = {key: {k: list(p.shape) for k, p in build(kind, kw).state_dict().items()} for key, (kind, kw) in PC.MANIFESTS.items()}
    with open(os.path.join(HERE, "state_dict_manifest_pose.json"), "w") as f:
        json.dump(manifest, f, indent=0, sort_keys=True)
    print(len(out), "arrays,", os.path.getsize(os.path.join(HERE, "kitti_pose.npz")), "bytes")


if __name__ == "__main__":
    main()
