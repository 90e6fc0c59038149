"""CPU: the pose restatement tests/pose_ref.py against the reference's own classes (tests/golden/kitti_pose.npz, written by
tests/golden/make_golden_pose.py) in float32 and float64; the pose modules' state_dict layout against the reference's
manifest; make_posenet's selection; and the argument validation of the four pose entry points, which needs no GPU."""
import json
import os
import types

import numpy as np
import pytest
import torch

import pose_cases as PC
import pose_ref as PR
from util import GOLDEN, assert_close, load_golden, sample
from wavelet_monodepth_amd import _lib, synth
from wavelet_monodepth_amd.kitti import PoseCNN, PoseDecoder, make_posenet

TOL = 2e-6    # tests/test_oracle_golden.py: the same torch build running the same operators in another order
DTYPES = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module")
def gold():
    return load_golden("kitti_pose.npz")


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("invert", [False, True])
def test_transform_vs_reference(gold, tag, invert):
    dtype = DTYPES[tag]
    v, t, g = PC.transform_case(PC.TRANSFORM_N)
    vv, tt = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (v, t))
    T = PR.transformation_from_parameters(vv[:, None], tt[:, None], invert)
    assert T.dtype == dtype and T.shape == (PC.TRANSFORM_N, 4, 4)
    (T * torch.from_numpy(g).to(dtype)).sum().backward()
    pre = "tf|%s|inv%d|" % (tag, invert)
    assert_close(T, gold[pre + "T"], TOL, "T")
    assert_close(vv.grad, gold[pre + "dv"], TOL, "d_axisangle")
    assert_close(tt.grad, gold[pre + "dt"], TOL, "d_translation")
    zero = ~v.any(1)
    assert zero.sum() >= 2
    for dv in (vv.grad.numpy(), gold[pre + "dv"]):                 # v = 0: no gradient reaches the axis-angle, exactly
        assert not dv[zero].any()
    sign = -1.0 if invert else 1.0
    assert np.array_equal(tt.grad.numpy()[zero], sign * g[zero][:, :3, 3].astype(tt.grad.numpy().dtype))


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("name", list(PC.NETS))
def test_networks_vs_reference(gold, name, tag):
    """values, the gradient of every input feature and of every parameter"""
    kind, kw, _ = PC.NETS[name]
    module = synth.fill_state_dict(PC.build(kind, kw), seed=PC.SEED)
    got = PC.run_net(PC.RefModule(module, kind, PC.frames_of(name), DTYPES[tag]), name, DTYPES[tag])
    want = {k.split("|", 2)[2]: v for k, v in gold.items() if k.startswith("%s|%s|" % (name, tag))}
    assert set(got) == set(want), set(got) ^ set(want)
    assert {"d" + k for k in module.state_dict()} <= set(got)
    for k, v in got.items():
        assert_close(v if k in ("axisangle", "translation") else sample(v, PC.SAMPLE), want[k], TOL, "%s %s %s" % (name, tag, k))


@pytest.mark.parametrize("key", list(PC.MANIFESTS))
def test_state_dict_manifest_and_strict_load(key, tmp_path):
    """the same keys and shapes as the reference's class, and a checkpoint written the reference's way
    (torch.save(model.state_dict())) loads with strict=True"""
    with open(os.path.join(GOLDEN, "state_dict_manifest_pose.json")) as f:
        want = json.load(f)[key]
    kind, kw = PC.MANIFESTS[key]
    m = PC.build(kind, kw)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == want
    ckpt = {k: torch.from_numpy(synth.uniform(tuple(s), k, 3)) for k, s in want.items()}
    path = str(tmp_path / "pose.pth")
    torch.save(ckpt, path)
    m.load_state_dict(torch.load(path), strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ckpt[k])


def test_pose_decoder_layout():
    m = PoseDecoder(np.array([64, 64, 128, 256, 512]), 2)
    assert list(m.convs) == ["squeeze", ("pose", 0), ("pose", 1), ("pose", 2)]
    assert all(type(c) is torch.nn.Conv2d for c in m.convs.values()) and list(m.net) == list(m.convs.values())
    assert m.num_frames_to_predict_for == 1 and m.convs[("pose", 0)].in_channels == 512
    assert PoseDecoder(np.array([64, 64, 128, 256, 512]), 1, 2).convs[("pose", 2)].out_channels == 12
    with pytest.raises(NotImplementedError):
        PoseDecoder(np.array([64, 64, 128, 256, 512]), 2, stride=2)


def test_make_posenet_selection():
    from wavelet_monodepth_amd.encoders import ResnetEncoder
    opts = types.SimpleNamespace(num_layers=18, weights_init="scratch", pose_model_type="separate_resnet", pose_model_input="pairs")
    depth_encoder = types.SimpleNamespace(num_ch_enc=np.array([64, 256, 512, 1024, 2048]))
    enc, dec = make_posenet(opts, depth_encoder, 2, 3)
    assert isinstance(enc, ResnetEncoder) and enc.encoder.conv1.in_channels == 6
    assert isinstance(dec, PoseDecoder) and (dec.num_input_features, dec.num_frames_to_predict_for) == (1, 2)
    assert dec.convs["squeeze"].in_channels == 512
    opts.pose_model_type = "shared"
    enc, dec = make_posenet(opts, depth_encoder, 2, 3)
    assert enc is None and isinstance(dec, PoseDecoder) and (dec.num_input_features, dec.num_frames_to_predict_for) == (2, 1)
    assert dec.convs["squeeze"].in_channels == 2048
    opts.pose_model_type = "posecnn"
    enc, dec = make_posenet(opts, depth_encoder, 2, 3)
    assert enc is None and isinstance(dec, PoseCNN) and dec.num_input_frames == 2
    opts.pose_model_input = "all"
    assert make_posenet(opts, depth_encoder, 3, 3)[1].num_input_frames == 3


def test_loss_options_defaults_and_layers_exports():
    from wavelet_monodepth_amd import layers, ops, photometric
    opt = photometric.LossOptions()
    assert (opt.pose_model_type, opt.pose_model_input) == ("separate_resnet", "pairs")
    assert layers.transformation_from_parameters is ops.transformation_from_parameters
    assert callable(layers.rot_from_axisangle) and callable(layers.get_translation_matrix) and callable(photometric.predict_poses)
    with pytest.raises(_lib.WmdError):
        ops.transformation_from_parameters(torch.zeros(2, 1, 3), torch.zeros(2, 1, 3))
    with pytest.raises(_lib.WmdError):
        ops.pose_head(torch.zeros(1, 8, 2, 2), torch.zeros(6, 8, 1, 1), torch.zeros(6), 1)


def test_pose_entry_points_validate_without_gpu():
    """a null pointer and a negative size are WMD_ERR_BAD_ARG, F outside 1..4 is WMD_ERR_UNSUPPORTED, before any HIP call
    (the dummy non-null pointers never reach a kernel)"""
    if not os.path.exists(_lib.LIB_PATH):
        from wavelet_monodepth_amd import build as b
        b.build()
    l = _lib.lib()
    p = 64
    assert l.wmd_pose_transform_fwd(None, p, p, 1, 0, None) == -1
    assert b"null" in l.wmd_last_error()
    assert l.wmd_pose_transform_fwd(p, p, None, 1, 0, None) == -1
    assert l.wmd_pose_transform_fwd(p, p, p, -1, 0, None) == -1
    assert b"N=-1" in l.wmd_last_error()
    assert l.wmd_pose_transform_bwd(p, p, None, p, p, 1, 0, None) == -1
    assert l.wmd_pose_transform_bwd(p, p, p, p, None, 1, 1, None) == -1
    assert l.wmd_pose_transform_bwd(p, p, p, p, p, -5, 0, None) == -1
    assert l.wmd_pose_head_fwd(None, p, p, p, p, p, 1, 8, 2, 2, 1, 0, 0.01, None) == -1
    assert l.wmd_pose_head_fwd(p, p, None, p, None, None, 1, 8, 2, 2, 1, 0, 0.01, None) == -1       # means is not optional
    assert l.wmd_pose_head_fwd(p, p, p, p, p, p, -1, 8, 2, 2, 1, 0, 0.01, None) == -1
    assert l.wmd_pose_head_fwd(p, p, p, p, p, p, 1, 8, 2, -2, 1, 0, 0.01, None) == -1
    for F in (0, 5, -1):
        assert l.wmd_pose_head_fwd(p, p, p, p, p, p, 1, 8, 2, 2, F, 0, 0.01, None) == -3
        assert b"F=" in l.wmd_last_error()
        assert l.wmd_pose_head_bwd(p, p, p, p, p, p, p, p, p, 1, 8, 2, 2, F, 0, 0.01, None) == -3
    assert l.wmd_pose_head_bwd(None, p, p, p, p, p, p, p, p, 1, 8, 2, 2, 1, 0, 0.01, None) == -1
    assert l.wmd_pose_head_bwd(p, p, p, None, None, p, p, p, p, 1, 8, 2, 2, 1, 0, 0.01, None) == -1  # neither gradient
    assert l.wmd_pose_head_bwd(p, p, p, p, None, p, p, p, None, 1, 8, 2, 2, 1, 0, 0.01, None) == -1  # no workspace
    assert l.wmd_pose_head_bwd(p, p, p, p, p, p, p, p, p, 1, -8, 2, 2, 1, 0, 0.01, None) == -1
