"""Value head and tanh-Normal actor (reference: algorithms/repo/models/actor_critic.py:9-102,
models/utils.py:112-166)."""
import torch
import torch.nn as nn

from .... import ops
from .decoder import _ScalarHead


VALUE_DISTS = ("normal", "twohot")


def value_dist_config(config):
    """config.value_dist and its three keys -> (name, bins, low, high).  value_dist: "normal" (the default:
    the reference's scalar head under a unit-variance Normal) or "twohot" (K logits over bins uniform in symlog space);
    value_bins (default 255) an integer in 2 .. 1024; value_bin_low / value_bin_high (-20.0 / 20.0) finite, low < high.  An
    unknown name or a value outside its range raises ValueError, whichever head is asked for."""
    import math
    import numbers

    name = getattr(config, "value_dist", "normal")
    if name not in VALUE_DISTS:
        raise ValueError(f'value_dist={name!r}: expected "normal" or "twohot"')
    bins = getattr(config, "value_bins", 255)
    if isinstance(bins, bool) or not isinstance(bins, numbers.Integral) or not 2 <= int(bins) <= 1024:
        raise ValueError(f"value_bins={bins!r}: expected an integer in 2 .. 1024")
    low, high = getattr(config, "value_bin_low", -20.0), getattr(config, "value_bin_high", 20.0)
    for key, v in (("value_bin_low", low), ("value_bin_high", high)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)):
            raise ValueError(f"{key}={v!r}: expected a finite number")
    if not float(low) < float(high):
        raise ValueError(f"value_bin_low={low!r}, value_bin_high={high!r}: expected low < high")
    return name, int(bins), float(low), float(high)


class ValueModel(_ScalarHead):
    """The scalar head (bins=None), or with config.value_dist = "twohot" the same trunk with `bins` logits in its last
    layer.  That layer's weight and bias are zeroed behind the usual draw, as DreamerV3 does: the head starts at uniform
    probabilities, a decoded value of exactly 0 for symmetric bins."""

    def __init__(self, belief_size, state_size, hidden_size, activation_function="relu", bins=None):
        super().__init__(belief_size, state_size, hidden_size, activation_function)
        self.bins = bins
        if bins is not None:
            # the scalar layer above has drawn what it always draws; the wide one draws under a forked generator, so
            # whatever is constructed behind this module initialises as it does with the scalar head
            with torch.random.fork_rng(devices=[]):
                self.fc4 = nn.Linear(hidden_size, int(bins))
            with torch.no_grad():
                self.fc4.weight.zero_()
                self.fc4.bias.zero_()

    def forward(self, belief, state):
        if self.bins is not None:
            raise NotImplementedError("the two-hot value head's logits are decoded by ops.twohot_decode (train_actor_critic)")
        return super().forward(belief, state)


class ActorModel(nn.Module):
    """230 -> hidden^4 -> 2A MLP (ELU, or ReLU when given explicitly); mean = mean_scale*tanh(m/mean_scale),
    std = softplus(s + init_std) + min_std; action ~ tanh(Normal(mean, std)).

    The reference passes `dense_activation_function` positionally into the `dist` slot
    (dreamer.py:99-105), leaving the activation at its default "elu"; the same signature is kept."""

    def __init__(self, belief_size, state_size, hidden_size, action_size, dist="tanh_normal",
                 activation_function="elu", min_std=0.1, init_std=0.0, mean_scale=5):
        super().__init__()
        self.act = ops.dense_act_id(activation_function, "ActorModel")
        self.fc1 = nn.Linear(belief_size + state_size, hidden_size)
        self.fc2 = nn.Linear(hidden_size, hidden_size)
        self.fc3 = nn.Linear(hidden_size, hidden_size)
        self.fc4 = nn.Linear(hidden_size, hidden_size)
        self.fc5 = nn.Linear(hidden_size, 2 * action_size)
        self._dist = dist
        self._min_std = min_std
        self._init_std = init_std
        self._mean_scale = mean_scale
        self._samples = 100  # SampleDist default (models/utils.py:138)

    def plist(self):
        return [t for m in (self.fc1, self.fc2, self.fc3, self.fc4, self.fc5) for t in (m.weight, m.bias)]

    @torch.no_grad()
    def forward(self, belief, state):
        feat = torch.cat([belief, state], dim=1).contiguous()
        raw, _ = ops.mlp_fwd([t.detach() for t in self.plist()], feat, act=self.act)
        mean, std, _ = ops.actor_head_fwd(raw, self._min_std, self._init_std, float(self._mean_scale))
        return mean, std

    @torch.no_grad()
    def get_action(self, belief, state, det=False, eps=None):
        """rsample of the policy (det=False) or SampleDist.mode (det=True): the sample with the
        highest log-probability among `_samples` draws (models/utils.py:149-158)."""
        feat = torch.cat([belief, state], dim=1).contiguous()
        raw, _ = ops.mlp_fwd([t.detach() for t in self.plist()], feat, act=self.act)
        if not det:
            if eps is None:
                eps = torch.randn(raw.shape[0], raw.shape[1] // 2, device=raw.device)
            S = state.shape[1]
            _, _, xsa = ops.actor_head_fwd(raw, self._min_std, self._init_std, float(self._mean_scale), eps=eps,
                                           state=feat[:, belief.shape[1]:])
            return xsa[:, S:].contiguous()
        from ..autograd import tanh_normal_mode

        mean, std, _ = ops.actor_head_fwd(raw, self._min_std, self._init_std, float(self._mean_scale))
        return tanh_normal_mode(mean, std, self._samples, eps)
