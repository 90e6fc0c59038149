"""CPU restatement of the pose path in stock torch ops, the reference the pose tests compare against (it is itself pinned to
the reference's classes by tests/golden/kitti_pose.npz, tests/test_pose_oracle.py).  Everything follows the dtype of its
inputs: float32 shows the reference's own rounding, float64 is the yardstick of the GPU tests.

  transformation_from_parameters(axisangle, translation, invert)      KITTI/layers.py:42-117
  pose_tail(x, w, b, frames)                                          conv1x1 -> mean over H, W -> 0.01 -> split
  pose_decoder(feature_lists, sd, frames) / pose_cnn(x, sd)           the two networks, `sd` keyed like their state_dicts
  predict_poses(inputs, features, models, opt)                        KITTI/trainer.py:254-310 with callables as models
  posecnn_transform(axisangle, translation, depth, frame_id)          KITTI/trainer.py:354-362
  generate_images_pred_posecnn(inputs, outputs, opt)                  oracle.photo_ref's warps with that branch
"""
import torch
import torch.nn.functional as F


def rotation(vec):
    """[N,3] axis-angle -> [N,3,3]: cos I + (1 - cos) a a^T + sin [a]x with a = v / (|v| + 1e-7), not renormalised"""
    angle = torch.norm(vec, 2, 1, True)                       # d|v|/dv = 0 at v = 0, as in the reference
    a = vec / (angle + 1e-7)
    ca, sa = torch.cos(angle)[:, :, None], torch.sin(angle)[:, :, None]
    zero = torch.zeros_like(a[:, 0])
    skew = torch.stack([zero, -a[:, 2], a[:, 1], a[:, 2], zero, -a[:, 0], -a[:, 1], a[:, 0], zero], 1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=vec.dtype).expand(vec.shape[0], 3, 3)
    return ca * eye + (1 - ca) * a[:, :, None] * a[:, None, :] + sa * skew


def transformation_from_parameters(axisangle, translation, invert=False):
    """[N,1,3] or [N,3] each -> [N,4,4]: [[R, t], [0, 1]], or its inverse [[R^T, -R^T t], [0, 1]]"""
    N = axisangle.shape[0]
    R, t = rotation(axisangle.reshape(N, 3)), translation.reshape(N, 3, 1)
    if invert:
        R = R.transpose(1, 2)
        t = -(R @ t)
    bottom = torch.tensor([0, 0, 0, 1], dtype=R.dtype).expand(N, 1, 4)
    return torch.cat([torch.cat([R, t], 2), bottom], 1)


def pose_tail(x, w, b, frames, scale=0.01):
    """x [B,C,H,W] -> (axisangle, translation) [B,frames,1,3], in the reference's order of operations"""
    out = F.conv2d(x, w.view(w.shape[0], -1, 1, 1), b).mean(3).mean(2)
    out = scale * out.view(-1, frames, 1, 6)
    return out[..., :3], out[..., 3:]


def pose_decoder(input_features, sd, frames):
    """PoseDecoder.forward on a list of feature lists; sd: net.0 (squeeze) ... net.3 (the 1x1 to 6 * frames)"""
    cat = torch.cat([F.relu(F.conv2d(f[-1], sd["net.0.weight"], sd["net.0.bias"])) for f in input_features], 1)
    out = F.relu(F.conv2d(cat, sd["net.1.weight"], sd["net.1.bias"], padding=1))
    out = F.relu(F.conv2d(out, sd["net.2.weight"], sd["net.2.bias"], padding=1))
    return pose_tail(out, sd["net.3.weight"], sd["net.3.bias"], frames)


POSECNN_GEOMETRY = ((7, 3), (5, 2), (3, 1), (3, 1), (3, 1), (3, 1), (3, 1))     # (kernel, padding), all of stride 2


def pose_cnn(x, sd):
    """PoseCNN.forward; sd: net.0 ... net.6 and pose_conv"""
    for i, (_, pad) in enumerate(POSECNN_GEOMETRY):
        x = F.relu(F.conv2d(x, sd["net.%d.weight" % i], sd["net.%d.bias" % i], stride=2, padding=pad))
    return pose_tail(x, sd["pose_conv.weight"], sd["pose_conv.bias"], sd["pose_conv.weight"].shape[0] // 6)


def predict_poses(inputs, features, models, opt):
    """models["pose"](pose_inputs) -> (axisangle, translation); models["pose_encoder"](images) -> feature list"""
    outputs = {}
    kind = opt.pose_model_type
    temporal = [f for f in opt.frame_ids if f != "s"]
    if opt.pose_model_input == "pairs" or len(opt.frame_ids) == 2:
        feats = {f: features[f] if kind == "shared" else inputs[("color_aug", f, 0)] for f in temporal}
        for f in temporal[1:]:
            pair = [feats[f], feats[0]] if f < 0 else [feats[0], feats[f]]
            if kind == "separate_resnet":
                pair = [models["pose_encoder"](torch.cat(pair, 1))]
            elif kind == "posecnn":
                pair = torch.cat(pair, 1)
            aa, tr = models["pose"](pair)
            outputs[("axisangle", 0, f)], outputs[("translation", 0, f)] = aa, tr
            outputs[("cam_T_cam", 0, f)] = transformation_from_parameters(aa[:, 0], tr[:, 0], invert=(f < 0))
    else:
        if kind == "shared":
            pose_inputs = [features[f] for f in temporal]
        else:
            pose_inputs = torch.cat([inputs[("color_aug", f, 0)] for f in temporal], 1)
            if kind == "separate_resnet":
                pose_inputs = [models["pose_encoder"](pose_inputs)]
        aa, tr = models["pose"](pose_inputs)
        for i, f in enumerate(opt.frame_ids[1:]):
            if f != "s":
                outputs[("axisangle", 0, f)], outputs[("translation", 0, f)] = aa, tr
                outputs[("cam_T_cam", 0, f)] = transformation_from_parameters(aa[:, i], tr[:, i])
    return outputs


def posecnn_transform(axisangle, translation, depth, frame_id):
    """the posecnn branch of generate_images_pred: the translation scaled by the mean inverse depth of the scale"""
    mean_inv_depth = (1 / depth).mean(3, True).mean(2, True)
    return transformation_from_parameters(axisangle[:, 0], translation[:, 0] * mean_inv_depth[:, 0], frame_id < 0)


def generate_images_pred_posecnn(inputs, outputs, opt):
    """oracle.photo_ref.generate_images_pred with the posecnn branch: the temporal frames are warped with the transform
    rebuilt per scale by posecnn_transform (not v1_multiscale, no depth hints)"""
    from oracle import photo_ref as P
    for scale in opt.loss_scales:
        disp = F.interpolate(outputs[("disp", scale)], [opt.height, opt.width], mode="bilinear", align_corners=False)
        _, depth = P.disp_to_depth(disp, opt.min_depth, opt.max_depth)
        outputs[("depth", 0, scale)] = depth
        for f in opt.frame_ids[1:]:
            T = inputs["stereo_T"] if f == "s" else posecnn_transform(outputs[("axisangle", 0, f)], outputs[("translation", 0, f)], depth, f)
            outputs[("color", f, scale)] = P.warp_frame(inputs[("color", f, 0)], depth, inputs[("K", 0)], inputs[("inv_K", 0)], T)
    return outputs
