"""PoseDecoder with the reference's name, constructor arguments and state_dict keys (KITTI/networks/decoders/pose_decoder.py):
squeeze 1x1 -> ReLU, two 3x3 + ReLU, then the 1x1 to 6 values per predicted frame, the spatial mean and the 0.01 scale.

The parameters live in plain nn.Conv2d holders (`net.0 ... net.3`); the holders' own forward is never used.  The three trunk
convolutions run on ops.conv2d_fused (ReLU = leaky with slope 0, zero padding), the tail on ops.pose_head: one launch for the
1x1, the mean, the scale, the axisangle / translation split and -- forward_transforms -- the 4x4 transform of every frame.
"""
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import ops
from ..layers import gated_backward_allowed

_RELU = dict(act="leaky", slope=0.0)


class PoseDecoder(nn.Module):
    def __init__(self, num_ch_enc, num_input_features, num_frames_to_predict_for=None, stride=1):
        super().__init__()
        if stride != 1:
            raise NotImplementedError("no factory of the reference passes a stride to PoseDecoder")
        self.num_ch_enc = num_ch_enc
        self.num_input_features = num_input_features
        if num_frames_to_predict_for is None:
            num_frames_to_predict_for = num_input_features - 1
        self.num_frames_to_predict_for = num_frames_to_predict_for

        self.convs = OrderedDict()
        self.convs[("squeeze")] = nn.Conv2d(int(self.num_ch_enc[-1]), 256, 1)
        self.convs[("pose", 0)] = nn.Conv2d(num_input_features * 256, 256, 3, stride, 1)
        self.convs[("pose", 1)] = nn.Conv2d(256, 256, 3, stride, 1)
        self.convs[("pose", 2)] = nn.Conv2d(256, 6 * num_frames_to_predict_for, 1)
        self.net = nn.ModuleList(list(self.convs.values()))

    def _trunk(self, input_features):
        last = [f[-1] for f in input_features]
        if len(last) != self.num_input_features:
            raise ValueError("PoseDecoder built for %d input features, got %d" % (self.num_input_features, len(last)))
        sq, p0, p1 = self.convs["squeeze"], self.convs[("pose", 0)], self.convs[("pose", 1)]
        # the same squeeze filter on every feature: one launch on the batch-stacked maps
        x = last[0] if len(last) == 1 else torch.cat(last, 0)
        x = ops.conv2d_fused(x, sq.weight, sq.bias, pad="zero", **_RELU)
        x1, x2 = x, None
        if len(last) > 1:
            parts = x.chunk(len(last), 0)
            x1 = parts[0]
            x2 = parts[1] if len(last) == 2 else torch.cat(parts[1:], 1)    # cat[x1, x2] is formed inside the convolution
        # ("pose", 0)'s output has one consumer, ("pose", 1), which returns its data gradient already multiplied by ReLU'
        gated = gated_backward_allowed(self)
        x = ops.conv2d_fused(x1, p0.weight, p0.bias, x2=x2, pad="zero", grad_is_dz=gated, **_RELU)
        return ops.conv2d_fused(x, p1.weight, p1.bias, pad="zero", x1_gate=("leaky", 0.0) if gated else None, **_RELU)

    def forward_transforms(self, input_features, invert_mask=0):
        """-> (axisangle, translation, T): T [B,F,4,4] = transformation_from_parameters of every predicted frame, frame f
        inverted when bit f of invert_mask is set, out of the pose head's own launch."""
        head = self.convs[("pose", 2)]
        return ops.pose_head(self._trunk(input_features), head.weight, head.bias, self.num_frames_to_predict_for,
                             invert_mask=invert_mask, scale=0.01)

    def forward(self, input_features):
        axisangle, translation, _ = self.forward_transforms(input_features)
        return axisangle, translation
