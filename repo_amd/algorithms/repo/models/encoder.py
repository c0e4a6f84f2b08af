"""Conv image encoder and the state-vector encoder (reference: algorithms/repo/models/encoder.py:6-47)."""
import torch
import torch.nn as nn

from .... import functional as Fn


def check_embedding_size(embedding_size):
    """config.embedding_size of the pixel stacks: any positive integer (1024: the encoder has no fc)."""
    if isinstance(embedding_size, bool) or int(embedding_size) != embedding_size or embedding_size < 1:
        raise ValueError(f"embedding_size must be a positive integer, not {embedding_size!r}")
    return int(embedding_size)


class VisualEncoder(nn.Module):
    """3x64x64 -> 32x31x31 -> 64x14x14 -> 128x6x6 -> 256x2x2 (k4, s2, ReLU), flattened to 1024, then
    `fc` = Identity if embedding_size == 1024 else Linear(1024, embedding_size), without an activation
    (reference models/encoder.py:30-32,40; image_size=128: -> 256x6x6, then fc 9216 -> embedding_size).

    The nn.Conv2d children are parameter containers only (same constructors, hence the same
    default initialisation and state_dict names as the reference); arithmetic runs in the HIP
    implicit-GEMM kernels.  Accepts float32 frames in [-1,1] or raw uint8 frames."""

    def __init__(self, embedding_size, activation_function="relu", image_size=64):
        """image_size=128: the BUILD-DEFINED wider stack of BASELINE config 4 (the reference's encoder hard-codes the
        64 x 64 flatten, encoder.py:39): the same four convs (3x128x128 -> ... -> 256x6x6) and `fc` =
        Linear(9216, embedding_size), applied without an activation like the reference's optional fc (:40)."""
        super().__init__()
        if activation_function != "relu":
            raise NotImplementedError("HIP encoder kernels fuse ReLU (cnn_activation_function='relu')")
        embedding_size = check_embedding_size(embedding_size)
        if image_size not in (64, 128):
            raise NotImplementedError(f"{image_size} x {image_size} frames: only 64 (the reference) and 128 (build-defined) are built")
        self.embedding_size = embedding_size
        self.image_size = image_size
        self.conv1 = nn.Conv2d(3, 32, 4, stride=2)
        self.conv2 = nn.Conv2d(32, 64, 4, stride=2)
        self.conv3 = nn.Conv2d(64, 128, 4, stride=2)
        self.conv4 = nn.Conv2d(128, 256, 4, stride=2)
        if image_size == 64:   # registered behind conv4 as in the reference: same default initialisation and state_dict order
            self.fc = nn.Identity() if embedding_size == 1024 else nn.Linear(1024, embedding_size)
        else:
            self.fc = nn.Linear(256 * 6 * 6, embedding_size)

    def plist(self):
        ps = [t for c in (self.conv1, self.conv2, self.conv3, self.conv4) for t in (c.weight, c.bias)]
        if isinstance(self.fc, nn.Linear):
            ps += [self.fc.weight, self.fc.bias]
        return ps

    def forward(self, observation):
        from ..autograd import encoder_apply

        return encoder_apply(self, observation)


MAX_OBSERVATION_SIZE = 1024   # state vectors of 1 .. 1024 floats (the contract of the symbolic modules)


def check_observation_size(observation_size, what):
    n = int(observation_size)
    if not 1 <= n <= MAX_OBSERVATION_SIZE:
        raise NotImplementedError(f"{what}: observation_size {n} is outside 1 .. {MAX_OBSERVATION_SIZE}, the widths the "
                                  "state-vector (pixel_obs=False) modules are built and tested for")
    return n


class SymbolicEncoder(nn.Module):
    """observation (n, obs) -> fc1 -> act -> fc2 -> act -> fc3 -> (n, embedding) (reference models/encoder.py:6-18): a
    dense chain on repo_mlp_fwd_act / repo_mlp_bwd_act.  Same children, shapes and construction order as the reference,
    hence the same default initialisation under a seed and the same state_dict.  activation_function "relu" or "elu"
    (config.cnn_activation_function, as the reference passes it), `self.act` its REPO_ACT_* id."""

    def __init__(self, observation_size, embedding_size, activation_function="relu"):
        super().__init__()
        from .... import ops

        self.act = ops.dense_act_id(activation_function, type(self).__name__)
        self.observation_size = check_observation_size(observation_size, type(self).__name__)
        self.embedding_size = embedding_size
        self.fc1 = nn.Linear(self.observation_size, embedding_size)
        self.fc2 = nn.Linear(embedding_size, embedding_size)
        self.fc3 = nn.Linear(embedding_size, embedding_size)

    def plist(self):
        return [t for m in (self.fc1, self.fc2, self.fc3) for t in (m.weight, m.bias)]

    def forward(self, observation):
        from ..autograd import dense_apply

        return dense_apply(self, observation)


def Encoder(symbolic, observation_size, embedding_size, activation_function="relu"):
    if symbolic:
        return SymbolicEncoder(observation_size, embedding_size, activation_function)
    return VisualEncoder(embedding_size, activation_function, image_size=int(observation_size[-1]))
