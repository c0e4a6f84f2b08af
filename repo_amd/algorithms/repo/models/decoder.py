"""Transposed-conv observation model, state-vector observation model and reward head
(reference: algorithms/repo/models/decoder.py:6-48,178-195)."""
import torch.nn as nn

from .encoder import check_embedding_size


class VisualObservationModel(nn.Module):
    """Linear(230->E) -> convT E->128 (k5) -> 64 (k5) -> 32 (k6) -> 3 (k6), stride 2, ReLU
    between; E = embedding_size (1024 by default).  Children hold parameters only; see repo_amd.functional.decoder_*."""

    def __init__(self, belief_size, state_size, embedding_size, activation_function="relu", image_size=64):
        """image_size=128 (build-defined, see VisualEncoder): conv4 becomes 32 -> 16 (k6, 30 -> 64, ReLU) and
        conv5 = 16 -> 3 (k2, 64 -> 128) is the output layer."""
        super().__init__()
        if activation_function != "relu":
            raise NotImplementedError("HIP decoder kernels fuse ReLU (cnn_activation_function='relu')")
        embedding_size = check_embedding_size(embedding_size)
        if image_size not in (64, 128):
            raise NotImplementedError(f"{image_size} x {image_size} frames: only 64 (the reference) and 128 (build-defined) are built")
        self.embedding_size = embedding_size
        self.image_size = image_size
        self.fc1 = nn.Linear(belief_size + state_size, embedding_size)
        self.conv1 = nn.ConvTranspose2d(embedding_size, 128, 5, stride=2)
        self.conv2 = nn.ConvTranspose2d(128, 64, 5, stride=2)
        self.conv3 = nn.ConvTranspose2d(64, 32, 6, stride=2)
        if image_size == 64:
            self.conv4 = nn.ConvTranspose2d(32, 3, 6, stride=2)
        else:
            self.conv4 = nn.ConvTranspose2d(32, 16, 6, stride=2)
            self.conv5 = nn.ConvTranspose2d(16, 3, 2, stride=2)

    def plist(self):
        mods = (self.fc1, self.conv1, self.conv2, self.conv3, self.conv4) + ((self.conv5,) if self.image_size == 128 else ())
        return [t for m in mods for t in (m.weight, m.bias)]

    def forward(self, belief, state):
        from ..autograd import decoder_apply

        return decoder_apply(self, belief, state)


class TIAObservationModel(nn.Module):
    """TIA's decoder (reference models/decoder.py:154-175): the visual decoder with a 6-channel output layer,
    returned as (recon, mask) = out.chunk(2, 1).  64 x 64 frames only (as the reference)."""

    def __init__(self, belief_size, state_size, embedding_size, activation_function="relu"):
        super().__init__()
        if activation_function != "relu":
            raise NotImplementedError("HIP decoder kernels fuse ReLU (cnn_activation_function='relu')")
        embedding_size = check_embedding_size(embedding_size)
        self.embedding_size = embedding_size
        self.fc1 = nn.Linear(belief_size + state_size, embedding_size)
        self.conv1 = nn.ConvTranspose2d(embedding_size, 128, 5, stride=2)
        self.conv2 = nn.ConvTranspose2d(128, 64, 5, stride=2)
        self.conv3 = nn.ConvTranspose2d(64, 32, 6, stride=2)
        self.conv4 = nn.ConvTranspose2d(32, 6, 6, stride=2)

    def plist(self):
        return [t for m in (self.fc1, self.conv1, self.conv2, self.conv3, self.conv4) for t in (m.weight, m.bias)]

    def forward(self, belief, state):
        from ..autograd import decoder_apply

        return decoder_apply(self, belief, state).chunk(2, 1)


class SymbolicObservationModel(nn.Module):
    """cat([belief, state]) -> fc1 -> act -> fc2 -> act -> fc3 -> (n, obs) (reference models/decoder.py:6-25).  Children
    hold parameters only; training ends in repo_linear_unit_nll (repo_amd.functional.symbolic_decoder_*).  Same children,
    shapes and construction order as the reference.  activation_function "relu" or "elu"
    (config.cnn_activation_function), `self.act` its REPO_ACT_* id."""

    def __init__(self, observation_size, belief_size, state_size, embedding_size, activation_function="relu"):
        super().__init__()
        from .... import ops
        from .encoder import check_observation_size

        self.act = ops.dense_act_id(activation_function, type(self).__name__)
        self.observation_size = check_observation_size(observation_size, type(self).__name__)
        self.embedding_size = embedding_size
        self.fc1 = nn.Linear(belief_size + state_size, embedding_size)
        self.fc2 = nn.Linear(embedding_size, embedding_size)
        self.fc3 = nn.Linear(embedding_size, self.observation_size)

    def plist(self):
        return [t for m in (self.fc1, self.fc2, self.fc3) for t in (m.weight, m.bias)]

    def forward(self, belief, state):
        from ..autograd import mlp_apply

        return mlp_apply(self, belief, state)


def ObservationModel(symbolic, observation_size, belief_size, state_size, embedding_size, activation_function="relu"):
    if symbolic:
        return SymbolicObservationModel(observation_size, belief_size, state_size, embedding_size, activation_function)
    return VisualObservationModel(belief_size, state_size, embedding_size, activation_function,
                                  image_size=int(observation_size[-1]))


class _ScalarHead(nn.Module):
    """230 -> hidden^3 -> 1 MLP on cat([belief, state]); activation_function "elu" or "relu" (the reference's default
    argument), `self.act` its REPO_ACT_* id."""

    def __init__(self, belief_size, state_size, hidden_size, activation_function="relu"):
        super().__init__()
        from .... import ops

        self.act = ops.dense_act_id(activation_function, type(self).__name__)
        self.fc1 = nn.Linear(belief_size + state_size, hidden_size)
        self.fc2 = nn.Linear(hidden_size, hidden_size)
        self.fc3 = nn.Linear(hidden_size, hidden_size)
        self.fc4 = nn.Linear(hidden_size, 1)

    def plist(self):
        return [t for m in (self.fc1, self.fc2, self.fc3, self.fc4) for t in (m.weight, m.bias)]

    def forward(self, belief, state):
        from ..autograd import mlp_apply

        return mlp_apply(self, belief, state).squeeze(dim=1)


REWARD_DISTS = ("normal", "twohot")


def reward_dist_config(config):
    """config.reward_dist and its three keys -> (name, bins, low, high), value_dist_config's rules
    (models/actor_critic.py) under the reward head's names.  reward_dist: "normal" (the default: the reference's scalar head
    under a unit-variance Normal) or "twohot" (K logits over bins uniform in symlog space); reward_bins (default 255) an
    integer in 2 .. 1024; reward_bin_low / reward_bin_high (-20.0 / 20.0) finite, low < high.  An unknown name or a value
    outside its range raises ValueError, whichever head is asked for."""
    import math
    import numbers

    name = getattr(config, "reward_dist", "normal")
    if name not in REWARD_DISTS:
        raise ValueError(f'reward_dist={name!r}: expected "normal" or "twohot"')
    bins = getattr(config, "reward_bins", 255)
    if isinstance(bins, bool) or not isinstance(bins, numbers.Integral) or not 2 <= int(bins) <= 1024:
        raise ValueError(f"reward_bins={bins!r}: expected an integer in 2 .. 1024")
    low, high = getattr(config, "reward_bin_low", -20.0), getattr(config, "reward_bin_high", 20.0)
    for key, v in (("reward_bin_low", low), ("reward_bin_high", high)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)):
            raise ValueError(f"{key}={v!r}: expected a finite number")
    if not float(low) < float(high):
        raise ValueError(f"reward_bin_low={low!r}, reward_bin_high={high!r}: expected low < high")
    return name, int(bins), float(low), float(high)


class RewardModel(_ScalarHead):
    """The scalar head (bins=None), or with config.reward_dist = "twohot" the same trunk with `bins` logits in its last
    layer, built as ValueModel(bins=...) builds its own (models/actor_critic.py): the scalar layer draws what it always
    draws, the wide one draws under a forked generator and is zeroed, so everything constructed behind this module
    initialises as with "normal" and a fresh head decodes to exactly 0."""

    def __init__(self, belief_size, state_size, hidden_size, activation_function="relu", bins=None):
        super().__init__(belief_size, state_size, hidden_size, activation_function)
        self.bins = bins
        if bins is not None:
            import torch

            with torch.random.fork_rng(devices=[]):
                self.fc4 = nn.Linear(hidden_size, int(bins))
            with torch.no_grad():
                self.fc4.weight.zero_()
                self.fc4.bias.zero_()

    def forward(self, belief, state):
        if self.bins is not None:
            raise NotImplementedError("the two-hot reward head's logits are decoded by ops.twohot_decode (train_actor_critic)")
        return super().forward(belief, state)


class ContinuationModel(_ScalarHead):
    """config.pcont: the continuation predictor of Hafner et al. 2020 (the reference has none).  The reward
    head's four layers; its output is the LOGIT of the probability that the episode goes on behind this latent."""
