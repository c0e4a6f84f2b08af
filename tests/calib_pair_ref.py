"""Plain-torch restatement of CalibratedRePo's calibration_mode="pair" step (reference algorithms/repo/repo_adapt.py:271-368:
the frozen scan over the 3 B columns [cal_src | cal_tgt | aln_tgt], the alignment loss, the two inverse-dynamics losses and
the encoder loss), written the way tests/calib_ref.py is: from the mathematics, on float64 leaves under autograd, noise
explicit.  The scan is oracle/repo_oracle.py:observe (ELU), the inverse-dynamics model and its masked NLL are
tests/inv_dyn_ref.py's, the discriminator's forward and the alignment loss tests/calib_ref.py's.
tests/test_calib_pair_cpu.py ties it to the reference's own pair_calibration.

make_pair_inputs holds the seeded inputs the goldens add to tests/calib_ref.py:make_calib_inputs: the actions and dones of
the aligned (target replay) batch and of the paired batch -- different ones, so that a swap shows -- and the scan's noise."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import repo_oracle as ro
from tests import calib_ref as cr
from tests import inv_dyn_ref as ir

# dones inside [1, L-1) of the goldens' L = 8, B = 4: both masks select some rows and drop others
ALN_DONES = ((3, 1), (5, 2))
CAL_DONES = ((2, 0), (4, 3), (6, 1))


def make_pair_inputs(L, B, A, S, u):
    """Step `u`: dict(aln_actions, aln_dones, cal_actions, cal_dones) -- (L, B, A) / (L, B, 1) float32 -- and the scan's
    noise OrderedDict(cal_prior, cal_post), each (L-1, 3B, S) in the reference's column order."""
    from oracle import fixtures as fx

    _, a_act, _, a_done = fx.make_batch(L, B, A, seed=51 + u, planted_dones=ALN_DONES, image=1)
    _, c_act, _, c_done = fx.make_batch(L, B, A, seed=71 + u, planted_dones=CAL_DONES, image=1)
    rs = np.random.RandomState(301 + u)
    noise = OrderedDict((k, rs.standard_normal((L - 1, 3 * B, S)).astype(np.float32)) for k in ("cal_prior", "cal_post"))
    return dict(aln_actions=a_act, aln_dones=a_done, cal_actions=c_act, cal_dones=c_done), noise


def selected(nonterms):
    """How many rows the loss of a (L, B, 1) nonterminal mask selects, and out of how many."""
    m = np.asarray(nonterms)[1:-1]
    return int((m == 1).sum()), int(m.size)


def scan(rssm, cal_src, cal_tgt, aln_tgt, cal_actions, cal_nonterms, aln_actions, aln_nonterms, eps_prior, eps_post):
    """Step 3: one observe scan from zeros over the columns [cal_src | cal_tgt | aln_tgt] ((L, B, E) embeddings each) on
    actions[:-1], embeds[1:], nonterms[:-1] -> (beliefs, posterior states), each (L-1, 3B, .)."""
    B = cal_src.shape[1]
    embeds = torch.cat((cal_src, cal_tgt, aln_tgt), 1)
    actions = torch.cat((cal_actions, cal_actions, aln_actions), 1)
    nonterms = torch.cat((cal_nonterms, cal_nonterms, aln_nonterms), 1)
    D = rssm["rnn.weight_hh"].shape[1]
    S = rssm["fc_state_prior.weight"].shape[0] // 2
    z = lambda w: torch.zeros(3 * B, w, dtype=embeds.dtype)  # noqa: E731
    outs = ro.observe(rssm, z(D), z(S), actions[:-1], embeds[1:], nonterms[:-1], eps_prior, eps_post)
    return outs[0], outs[4]


def inv_nll(inv, act, beliefs_in, states_in, beliefs_out, actions, nonterms, min_std=0.1):
    """Steps 5 / 6: rows x = [beliefs_in_t | states_in_t | beliefs_out_t+1], t < T-1, through the inverse-dynamics model;
    the mean NLL of actions[1:-1] over the rows with nonterms[1:-1] == 1 (NaN when none is selected, like the reference)."""
    x = torch.cat((beliefs_in[:-1], states_in[:-1], beliefs_out[1:]), dim=2).flatten(0, 1)
    _, _, raw = ir.model(inv, x, act, None, min_std)
    total, count = ir.masked_nll(raw, actions[1:-1].flatten(0, 1), nonterms[1:-1].flatten(), min_std)
    return total / count if count else total * float("nan")


def latent_losses(rssm, inv, act, cal_src, cal_tgt, aln_tgt, cal_actions, cal_nonterms, aln_actions, aln_nonterms,
                  eps_prior, eps_post):
    """Steps 3, 5 and 6 -> (dyn_loss, calib_loss)."""
    B = cal_src.shape[1]
    beliefs, posts = scan(rssm, cal_src, cal_tgt, aln_tgt, cal_actions, cal_nonterms, aln_actions, aln_nonterms,
                          eps_prior, eps_post)
    (sb, tb, ab), (sp, _, ap) = beliefs.split(B, 1), posts.split(B, 1)
    dyn = inv_nll(inv, act, ab, ap, ab, aln_actions, aln_nonterms)
    calib = inv_nll(inv, act, sb, sp, tb, cal_actions, cal_nonterms)
    return dyn, calib


def encoder_loss(rssm, inv, act, disc, support, cal_src, cal_tgt, aln_tgt, cal_actions, cal_nonterms, aln_actions,
                 aln_nonterms, eps_prior, eps_post, eps_tgt, coefs=(1.0, 1.0, 1.0)):
    """Steps 3-7 with `disc` the discriminator AFTER its step (tests/calib_ref.py restates the step itself):
    -> dict(aln, dyn, calib, encoder) with encoder = aln_coef aln + dyn_coef dyn + calib_coef calib."""
    d_tgt, _, _ = cr.disc_forward(disc, aln_tgt.flatten(0, 1), eps_tgt)
    aln = cr.generator_loss(d_tgt, support)
    dyn, calib = latent_losses(rssm, inv, act, cal_src, cal_tgt, aln_tgt, cal_actions, cal_nonterms, aln_actions,
                               aln_nonterms, eps_prior, eps_post)
    return dict(aln=aln, dyn=dyn, calib=calib, encoder=coefs[0] * aln + coefs[1] * dyn + coefs[2] * calib)
