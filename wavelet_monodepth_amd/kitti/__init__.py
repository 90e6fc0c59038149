from .depth_decoder import DepthDecoder, DepthWaveProgressiveDecoder  # noqa: F401
from .sparse_decoder import SparseDepthWaveProgressiveDecoder  # noqa: F401
from .pose_decoder import PoseDecoder  # noqa: F401
from .pose_cnn import PoseCNN  # noqa: F401
from .network_constructors import make_depth_decoder, make_depth_encoder, make_posenet  # noqa: F401
