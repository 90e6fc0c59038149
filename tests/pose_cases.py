"""Inputs of the pose tests, shared by tests/golden/make_golden_pose.py (the reference's classes), tests/test_pose_oracle.py
(pose_ref against the fixture) and tests/test_gpu_pose.py (the kernels): everything is drawn from synth, so the fixture
stores outputs only."""
import numpy as np
import torch

from wavelet_monodepth_amd import synth

R18_LAST, R50_LAST = 512, 2048
SAMPLE = 512      # stored entries per gradient tensor (util.sample strides)

# name -> (kind, constructor arguments, input shapes)
NETS = {
    "dec_r18_f2": ("decoder", dict(num_ch_enc=[64, 64, 128, 256, R18_LAST], num_input_features=2), [(2, R18_LAST, 2, 2)] * 2),
    "dec_r50_f1x2": ("decoder", dict(num_ch_enc=[64, 256, 512, 1024, R50_LAST], num_input_features=1, num_frames_to_predict_for=2),
                     [(2, R50_LAST, 2, 2)]),
    "dec_r18_6x20": ("decoder", dict(num_ch_enc=[64, 64, 128, 256, R18_LAST], num_input_features=2), [(2, R18_LAST, 6, 20)] * 2),
    "cnn2": ("cnn", dict(num_input_frames=2), [(2, 6, 64, 64)]),
}
MANIFESTS = {"PoseDecoder|r18,2": ("decoder", dict(num_ch_enc=[64, 64, 128, 256, R18_LAST], num_input_features=2)),
             "PoseDecoder|r50,1,2": ("decoder", dict(num_ch_enc=[64, 256, 512, 1024, R50_LAST], num_input_features=1,
                                                     num_frames_to_predict_for=2)),
             "PoseCNN|2": ("cnn", dict(num_input_frames=2)), "PoseCNN|3": ("cnn", dict(num_input_frames=3))}
SEED = 23


def build(kind, kw):
    """a pose network of the package from a NETS / MANIFESTS entry"""
    from wavelet_monodepth_amd.kitti import PoseCNN, PoseDecoder
    if kind == "cnn":
        return PoseCNN(**kw)
    return PoseDecoder(np.array(kw["num_ch_enc"]), **{k: v for k, v in kw.items() if k != "num_ch_enc"})


class RefModule:
    """pose_ref behind the call signature run_net expects, on the parameters of one of our modules at a chosen dtype"""

    def __init__(self, module, kind, frames, dtype):
        self.sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in module.state_dict().items()}
        self.kind, self.frames = kind, frames

    def named_parameters(self):
        return self.sd.items()

    def __call__(self, x):
        import pose_ref as PR
        return PR.pose_cnn(x, self.sd) if self.kind == "cnn" else PR.pose_decoder(x, self.sd, self.frames)


def frames_of(name):
    kind, kw, _ = NETS[name]
    if kind == "cnn":
        return kw["num_input_frames"] - 1
    return kw.get("num_frames_to_predict_for") or kw["num_input_features"] - 1


def net_inputs(name):
    """float32 numpy inputs of a network: encoder-like features (non-negative, as after a ReLU) or images in [0, 1)"""
    kind, _, shapes = NETS[name]
    if kind == "cnn":
        return [synth.uniform(s, "%s_in%d" % (name, i), SEED, 0.0, 1.0) for i, s in enumerate(shapes)]
    return [np.maximum(synth.normal(s, "%s_in%d" % (name, i), SEED), 0.0) for i, s in enumerate(shapes)]


def out_weights(name):
    """upstream gradients of (axisangle, translation) [B,F,1,3]"""
    B, F = NETS[name][2][0][0], frames_of(name)
    return [synth.uniform((B, F, 1, 3), "%s_g%s" % (name, k), SEED) for k in ("a", "t")]


def run_net(module, name, dtype, device="cpu"):
    """forward + backward of a pose network module (the reference's, or ours on the GPU) -> dict of float64 numpy arrays:
    axisangle, translation, din<i>, and d<parameter name> for every parameter"""
    kind = NETS[name][0]
    xs = [torch.from_numpy(a).to(device, dtype).requires_grad_(True) for a in net_inputs(name)]
    aa, tr = module(xs[0]) if kind == "cnn" else module([[x] for x in xs])
    ga, gt = (torch.from_numpy(g).to(device, dtype) for g in out_weights(name))
    ((aa * ga).sum() + (tr * gt).sum()).backward()
    out = {"axisangle": aa, "translation": tr}
    out.update(("din%d" % i, x.grad) for i, x in enumerate(xs))
    out.update(("d" + k, p.grad) for k, p in module.named_parameters())
    return {k: v.detach().cpu().double().numpy() for k, v in out.items()}


def transform_case(N, seed=SEED):
    """axisangle, translation [N,3] and an upstream gradient [N,4,4]: unit directions scaled to the angles 0 (exactly), 1e-8
    (below the 1e-7 of the axis), 1e-3, 0.1, 3.0 and pi in turn; translations in [-1, 1)."""
    d = synth.normal((N, 3), "tf_dir", seed).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    angles = np.array([0.0, 1e-8, 1e-3, 0.1, 3.0, np.pi])[np.arange(N) % 6]
    v = (d * angles[:, None]).astype(np.float32)
    v[angles == 0.0] = 0.0
    return v, synth.uniform((N, 3), "tf_t", seed), synth.uniform((N, 4, 4), "tf_g", seed)


TRANSFORM_N = 13      # the fixture's rows: every angle twice, and one more zero
