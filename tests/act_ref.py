"""Plain-torch restatement of the RSSM cell, the rollout step and the MLP heads with the dense activation as a parameter
("elu" / "relu": the reference's act_fn = getattr(F, activation_function), models/rssm.py:24, decoder.py:178-195,
actor_critic.py:9-26).  oracle/repo_oracle.py hard-codes F.elu; tests/test_dense_act_cpu.py ties this module's ELU form to
it.  Run it on float64 leaves under autograd.

Every function takes `pre`, a list that receives each ReLU pre-activation it forms (detached): a ReLU pre-activation
within rounding of zero has no agreed derivative, so the tests assert min |pre| >= PRE_MARGIN before they compare (ELU
is smooth enough at zero -- value and derivative are continuous -- and records nothing)."""
import torch
import torch.nn.functional as F

ACTS = {"elu": F.elu, "relu": F.relu}
PRE_MARGIN = 1e-4


def _dense(act, x, w, b, pre):
    z = F.linear(x, w, b)
    if pre is not None and act == "relu":
        pre.append(z.detach())
    return ACTS[act](z)


def min_abs_pre(pre):
    return min((float(z.abs().min()) for z in pre), default=float("inf"))


def gru_cell(p, x, h):
    gi = F.linear(x, p["rnn.weight_ih"], p["rnn.bias_ih"])
    gh = F.linear(h, p["rnn.weight_hh"], p["rnn.bias_hh"])
    H = h.shape[1]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h


def compute_belief(p, prev_belief, state, action, act, pre=None):
    hid = _dense(act, torch.cat([state, action], 1), p["fc_embed_state_action.weight"], p["fc_embed_state_action.bias"], pre)
    return gru_cell(p, hid, prev_belief)


def gaussian_head(p, prefix_embed, prefix_state, x, eps, act, pre=None, min_std=0.1):
    hid = _dense(act, x, p[prefix_embed + ".weight"], p[prefix_embed + ".bias"], pre)
    out = F.linear(hid, p[prefix_state + ".weight"], p[prefix_state + ".bias"])
    S = out.shape[1] // 2
    mean, raw = out[:, :S], out[:, S:]
    std = F.softplus(raw) + min_std
    return mean + std * eps, mean, std


def observe(p, prev_belief, prev_state, actions, embeds, nonterms, eps_prior, eps_post, act, pre=None):
    """-> [beliefs, prior_states, prior_means, prior_stds, post_states, post_means, post_stds], each (T, B, .)."""
    outs = [[] for _ in range(7)]
    belief, post = prev_belief, prev_state
    for t in range(actions.shape[0]):
        belief = compute_belief(p, belief, post * nonterms[t], actions[t], act, pre)
        prior, pm, ps = gaussian_head(p, "fc_embed_belief_prior", "fc_state_prior", belief, eps_prior[t], act, pre)
        post, qm, qs = gaussian_head(p, "fc_embed_belief_posterior", "fc_state_posterior",
                                     torch.cat([belief, embeds[t]], 1), eps_post[t], act, pre)
        for lst, v in zip(outs, (belief, prior, pm, ps, post, qm, qs)):
            lst.append(v)
    return [torch.stack(o, 0) for o in outs]


def mlp_head(p, x, n_layers, act, pre=None):
    h = x
    for i in range(1, n_layers):
        h = _dense(act, h, p[f"fc{i}.weight"], p[f"fc{i}.bias"], pre)
    return F.linear(h, p[f"fc{n_layers}.weight"], p[f"fc{n_layers}.bias"])


def actor_fwd(p, belief, state, act, pre=None, min_std=0.1, init_std=0.0, mean_scale=5.0):
    out = mlp_head(p, torch.cat([belief, state], 1), 5, act, pre)
    A = out.shape[1] // 2
    return mean_scale * torch.tanh(out[:, :A] / mean_scale), F.softplus(out[:, A:] + init_std) + min_std, out


def imagine(rssm, actor, belief0, state0, horizon, eps_act, eps_prior, rssm_act, actor_act, pre=None):
    """-> [beliefs, states, prior_means, prior_stds, actor raw outputs]; the RSSM layers run `rssm_act`, the actor trunk
    `actor_act` (the agents: always "elu", whatever the config says)."""
    beliefs, states, means, stds, raws = [], [], [], [], []
    belief, state = belief0, state0
    for t in range(horizon - 1):
        a_mean, a_std, raw = actor_fwd(actor, belief.detach(), state.detach(), actor_act, pre)
        action = torch.tanh(a_mean + a_std * eps_act[t])
        belief = compute_belief(rssm, belief, state, action, rssm_act, pre)
        state, pm, ps = gaussian_head(rssm, "fc_embed_belief_prior", "fc_state_prior", belief, eps_prior[t], rssm_act, pre)
        for lst, v in zip((beliefs, states, means, stds, raws), (belief, state, pm, ps, raw)):
            lst.append(v)
    return [torch.stack(x, 0) for x in (beliefs, states, means, stds, raws)]
