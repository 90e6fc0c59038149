"""PoseCNN with the reference's name, constructor argument and state_dict keys (KITTI/networks/pose_cnn.py): seven strided
convolutions + ReLU on the concatenated frames (plain torch.nn, like the encoders), then the 1x1 `pose_conv`, the spatial mean
and the 0.01 scale on ops.pose_head (one launch, with the 4x4 transforms on request)."""
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class PoseCNN(nn.Module):
    def __init__(self, num_input_frames):
        super().__init__()
        self.num_input_frames = num_input_frames
        self.convs = {}
        self.convs[0] = nn.Conv2d(3 * num_input_frames, 16, 7, 2, 3)
        self.convs[1] = nn.Conv2d(16, 32, 5, 2, 2)
        self.convs[2] = nn.Conv2d(32, 64, 3, 2, 1)
        self.convs[3] = nn.Conv2d(64, 128, 3, 2, 1)
        self.convs[4] = nn.Conv2d(128, 256, 3, 2, 1)
        self.convs[5] = nn.Conv2d(256, 256, 3, 2, 1)
        self.convs[6] = nn.Conv2d(256, 256, 3, 2, 1)
        self.pose_conv = nn.Conv2d(256, 6 * (num_input_frames - 1), 1)
        self.num_convs = len(self.convs)
        self.net = nn.ModuleList(list(self.convs.values()))

    def forward_transforms(self, out, invert_mask=0):
        """-> (axisangle, translation, T [B,F,4,4]), frame f inverted when bit f of invert_mask is set"""
        for i in range(self.num_convs):
            out = F.relu(self.convs[i](out))
        return ops.pose_head(out, self.pose_conv.weight, self.pose_conv.bias, self.num_input_frames - 1, invert_mask=invert_mask,
                             scale=0.01)

    def forward(self, out):
        axisangle, translation, _ = self.forward_transforms(out)
        return axisangle, translation
