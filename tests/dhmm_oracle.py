"""CPU restatement of the driven-HMM forward-backward recursion (the reference's models/dHMM.py:42-78), used by the tests
at sizes the golden fixtures (tests/golden/dhmm.npz) do not cover; tests/test_dhmm_host.py pins it to those fixtures.

Conventions as in the reference: time first, obs (T, lead, K), tr (T, lead, K, K) with row = from-state and column =
to-state, init (batch, K) broadcast against lead.  The log-sum-exp is max + log(sum(exp(x - max))), so a reduction over a
set of -inf yields NaN exactly where the reference's does.
"""
import torch


def lse(x, dims, keepdim=False):
    """max + log sum exp(x - max) over dims (the reference's utils/torch_functions.py:2-4)"""
    m = x.amax(dims, keepdim=True)
    return m.amax(dims, keepdim) + (x - m).exp().sum(dim=dims, keepdim=keepdim).log()


def forward_backward(obs, tr, init, ptemp=1.0):
    """Returns p (T, lead, K), SEzz (T, lead, K, K) per step, SEz0 (lead, K) and logZ (lead)."""
    T = obs.shape[0]
    f = obs.clone()
    # step 0 leaves a virtual state drawn from init (:47)
    f[0] = lse(obs[0].unsqueeze(-2) + init.unsqueeze(-1) + tr[0], -2)
    # filtering without per-step normalisation (:49-51)
    for t in range(1, T):
        f[t] = lse(f[t - 1].unsqueeze(-1) + obs[t].unsqueeze(-2) + tr[t], -2)
    logZ = lse(f[-1], -1, True)
    f = f - logZ  # every filtered message shifted by the same constant (:54)
    logZ = logZ.squeeze(-1)
    SEzz = torch.zeros(tuple(f.shape) + (f.shape[-1],), dtype=f.dtype)

    def pair_logits(src, step_tr, smoothed):
        # xi_ij = (src_i + tr_ij - lse_i(src_i + tr_ij)) + smoothed_j
        a = src.unsqueeze(-1) + step_tr
        return (a - lse(a, -2, True)) + smoothed.unsqueeze(-2)

    # smoothing, overwriting the filtered message at t by the smoothed one (:57-63)
    for t in range(T - 2, -1, -1):
        xi = pair_logits(f[t], tr[t + 1], f[t + 1])
        f[t] = lse(xi, -1)
        SEzz[t + 1] = (xi - lse(xi, (-1, -2), True)).exp()
    # the virtual initial state (:65-70)
    xi = pair_logits(init, tr[0], f[0])
    s0 = lse(xi, -1)
    SEz0 = (s0 - lse(s0, -1, True)).exp()
    SEzz[0] = (xi - lse(xi, (-1, -2), True)).exp()
    p = ((f - f.max(-1, keepdim=True)[0]) / ptemp).exp()
    p = p / p.sum(-1, keepdim=True)
    return p, SEzz, SEz0, logZ


def golden_inputs(c):
    """(obs, tr, init) of a kernel case of tests/golden/dhmm.npz: the operands are stored as int8 grids q with a
    power-of-two step (q = -128 encodes -inf), so step * q is the exact fp64 value the reference ran on"""
    def decode(q, step):
        return torch.where(q == -128, torch.full(q.shape, -float("inf"), dtype=torch.float64), q.double() * float(step))
    return decode(c["obs_q"], c["obs_grid"]), decode(c["tr_q"], c["tr_grid"]), c["init"]


def golden_outputs(c, p, SEzz):
    """the stored p / SEzz of a kernel case and the matching slices of computed ones: cases with a "_head" field keep the
    first series only (SEz0 and logZ are always complete)"""
    if "p_head" in c:
        h = c["p_head"].shape[1]
        return (p[:, :h], c["p_head"]), (SEzz[:, :h], c["SEzz_head"])
    return (p, c["p"]), (SEzz, c["SEzz"])
