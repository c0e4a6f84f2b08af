"""MLP (reference common/models/mlps.py:11-32): Linear layers with an activation between and after them, on the HIP dense
kernels.  State-dict keys (`layers.{0,2,...}.{weight,bias}`), construction order and initialisation (orthogonal weights,
zero biases: common/models/utils.py:102-106) are the reference's, so a seed gives the same parameters.

Built: act "ReLU" with equal hidden widths (ops.mlp_fwd / mlp_bwd at ACT_RELU: CalibratedRePo's density-ratio model
log_tau) and "LeakyReLU" (functional.leaky_chain_*: the VDB discriminator's encoder); output_act "Identity".
"""
import torch
import torch.nn as nn

from ... import functional as Fn
from ... import ops


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dims, output_dim, act="ReLU", output_act="Identity"):
        super().__init__()
        if act not in ("ReLU", "LeakyReLU") or output_act != "Identity":
            raise NotImplementedError(f"MLP: built for act 'ReLU' / 'LeakyReLU' and output_act 'Identity', not {act!r} / {output_act!r}")
        if act == "ReLU" and len(set(hidden_dims)) > 1:
            raise NotImplementedError("MLP(act='ReLU'): built for equal hidden widths")
        self.act_name = act
        layers = []
        curr_dim = input_dim
        for dim in hidden_dims:
            layers.append(nn.Linear(curr_dim, dim))
            layers.append(getattr(nn, act)())
            curr_dim = dim
        layers.append(nn.Linear(curr_dim, output_dim))
        layers.append(nn.Identity())
        self.layers = nn.Sequential(*layers)
        for m in self.layers:
            if isinstance(m, nn.Linear):
                nn.init.orthogonal_(m.weight)
                nn.init.zeros_(m.bias)

    def plist(self):
        return [t for m in self.layers if isinstance(m, nn.Linear) for t in (m.weight, m.bias)]

    def fwd(self, x):
        """-> (out, hidden activations) for `bwd`; x (N, input_dim) with contiguous rows."""
        p = [t.detach() for t in self.plist()]
        if self.act_name == "ReLU":
            return ops.mlp_fwd(p, x, act=ops.ACT_RELU)
        return Fn.leaky_chain_fwd(p, x)

    def bwd(self, x, hid, dout, dparams=None, accumulate=False, dx=None):
        p = [t.detach() for t in self.plist()]
        if self.act_name == "ReLU":
            ops.mlp_bwd(p, x, hid, dout, dparams=dparams, accumulate_w=accumulate, dx=dx, act=ops.ACT_RELU)
        else:
            Fn.leaky_chain_bwd(p, x, hid, dout, dparams=dparams, accumulate=accumulate, dx=dx)

    @torch.no_grad()
    def forward(self, x):
        return self.fwd(x.float().contiguous())[0]
