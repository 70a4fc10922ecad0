#!/usr/bin/env python3
"""Generate tests/golden/dhmm.npz by RUNNING the reference's driven HMM (models/dHMM.py).

Same rules as tools/gen_golden.py (whose Book / quiet helpers it reuses): it runs only where the reference is
available, imports it, and stores nothing but DATA -- the inputs fed to a reference method and the tensors it returned
or left in its attributes.  Seeded; a rerun reproduces the file bit for bit.

    python tools/gen_golden_dhmm.py

Kernel cases ("fb_*") call forward_backward_loop directly on random observation and transition logits.  Class cases
("cls_*") run dHMM.raw_update on data drawn as in the reference's tests/test_models.py:134-165, with the random initial
state (NIW mu, the MNLR coefficient posterior incl. its ARD Gamma
factor) stored as inputs.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (sets fp64 as the default dtype and puts the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dists  # noqa: E402  (reference)


def _model(K, p, batch=(), ptemp=1.0):
    from models.dHMM import dHMM  # reference
    obs = dists.NormalInverseWishart(event_shape=(2,), batch_shape=tuple(batch) + (K,))
    return dHMM(obs_dist=obs, p=p, ptemp=ptemp)


def quantize(x, scale):
    """x on the grid scale * q, q an int8 in [-127, 127] (-128 encodes -inf); scale is a power of two, so scale * q is exact in
    fp32 and fp64 and the fixture stores one byte per operand entry"""
    q = torch.clamp(torch.round(x / scale), -127, 127)
    q = torch.where(torch.isneginf(x), torch.full_like(q, -128), q).to(torch.int8)
    return q, torch.where(q == -128, torch.full_like(x, -torch.inf), q.double() * scale)


def fb_case(b, name, K, T, S, gen, batch=(), ptemp=1.0, obs_scale=2.0, tr_scale=1.5, keep=None, head=None,
            obs_grid=1 / 16, tr_grid=1 / 8):
    """keep: fraction of allowed transitions per (step, chain); a cycle i -> i+1 stays allowed, so every state is
    reachable and every state has a successor.  The operands are stored as int8 grids (quantize); the reference ran on
    exactly the decoded values.  head: store p and the per-step pair posteriors of the first `head` series only (fields
    p_head, SEzz_head; SEz0 and logZ stay complete) to keep the fixture small."""
    b.begin(name)
    with gg.quiet():
        m = _model(K, 3, batch, ptemp)
    m.initial.alpha = m.initial.alpha_0 + 2.0 * torch.rand(tuple(batch) + (K,), generator=gen)
    lead = (S,) + tuple(batch)
    obs = obs_scale * torch.randn((T,) + lead + (K,), generator=gen)
    tr = torch.log_softmax(tr_scale * torch.randn((T,) + lead + (K, K), generator=gen), -1)
    if keep is not None:
        mask = torch.rand((T,) + lead + (K, K), generator=gen) < keep
        mask |= torch.eye(K, dtype=torch.bool).roll(1, -1)
        tr = torch.where(mask, tr, torch.full_like(tr, -torch.inf))
    obs_q, obs = quantize(obs, obs_grid)
    tr_q, tr = quantize(tr, tr_grid)
    for k, v in (("K", K), ("T", T), ("ptemp", ptemp), ("obs_grid", obs_grid), ("tr_grid", tr_grid)):
        b.put(k, v)
    b.put("batch_shape", np.array(batch, dtype=np.int64))
    b.put("obs_q", obs_q)
    b.put("tr_q", tr_q)
    b.put("init", m.initial.loggeomean())
    with gg.quiet():
        SEzz, SEz0, logZ = m.forward_backward_loop(obs.clone(), tr)
    if head is None:
        b.put("p", m.p)
        b.put("SEzz", SEzz)
    else:
        b.put("p_head", m.p[:, :head])
        b.put("SEzz_head", SEzz[:, :head])
    b.put("SEz0", SEz0)
    b.put("logZ", logZ)


def synth(T, S, K, d, p, gen):
    """switching data driven by an input, as the reference's tests/test_models.py:143-161"""
    A = torch.rand(K, K, generator=gen) + 5 * torch.eye(K)
    A = A / A.sum(-1, keepdim=True)
    B = 2 * torch.randn(K, d, generator=gen)
    Cm = torch.randn(K, p, K, generator=gen) / np.sqrt(p)
    X = torch.randn(T, S, p, 1, generator=gen)
    z = torch.rand(T, S, K, generator=gen).argmax(-1)
    Y = torch.randn(T, S, d, generator=gen)
    for t in range(1, T):
        z[t] = (A[z[t - 1]].log() + (X[t] * Cm[z[t - 1]]).sum(-2) + torch.randn(S, K, generator=gen)).argmax(-1)
        Y[t] = B[z[t]] + torch.randn(S, d, generator=gen) / 10.0
    return X.squeeze(-1), Y


def cls_case(b, name, X, Y, K, p, iters, lr, gen):
    b.begin(name)
    d = Y.shape[-1]
    torch.manual_seed(int(torch.randint(0, 2 ** 31, (1,), generator=gen)))
    from models.dHMM import dHMM  # reference
    with gg.quiet():
        m = dHMM(obs_dist=dists.NormalInverseWishart(event_shape=(d,), batch_shape=(K,)), p=p)
    for k, v in (("K", K), ("xdim", p), ("iters", iters), ("lr", lr)):
        b.put(k, v)
    b.put("init_niw_mu", m.obs_dist.mu)
    gg.snap_ard(b, m.transition.beta, "init_beta_")  # the gate's coefficients and their ARD Gamma factor start at random
    with gg.quiet():
        m.raw_update(X, Y, iters=iters, lr=lr)
    gg.snap_niw(b, m.obs_dist, "niw_")
    b.put("beta_mu", m.transition.beta.mu)
    b.put("beta_invSigma", m.transition.beta.invSigma)
    b.put("initial_alpha", m.initial.alpha)
    b.put("p", m.p)
    b.put("SEzz", m.SEzz)
    b.put("SEz0", m.SEz0)
    b.put("NA", m.NA)
    b.put("logZ", m.logZ)
    b.put("sumlogZ", m.sumlogZ)
    b.put("KLqprior", m.KLqprior())
    b.put("ELBO", m.ELBO())


def gen_dhmm():
    b = gg.Book()
    gen = torch.Generator().manual_seed(1616)
    torch.manual_seed(16)
    fb_case(b, "fb_k4_T100_S199", 4, 100, 199, gen, head=2, obs_scale=1.0, tr_scale=0.75, obs_grid=1 / 2, tr_grid=1.0)  # the reference test's size
    fb_case(b, "fb_k25", 25, 6, 3, gen, head=1)
    fb_case(b, "fb_k2_T2", 2, 2, 5, gen)
    fb_case(b, "fb_k9_T1", 9, 1, 3, gen)
    fb_case(b, "fb_k5_ptemp", 5, 20, 4, gen, ptemp=2.5)
    fb_case(b, "fb_k3_b2", 3, 15, 4, gen, batch=(2,))                     # two initial distributions (NB = 2)
    fb_case(b, "fb_k6_forbidden", 6, 25, 5, gen, keep=0.4)                # -inf transitions, every state reachable
    fb_case(b, "fb_k5_peaked", 5, 40, 4, gen, obs_scale=300.0, tr_scale=30.0, obs_grid=8.0, tr_grid=2.0)  # sharply peaked
    # the class cases share one data set (case "cls_data"); X and Y are rounded to fp32-representable values
    K, p = 4, 10
    X, Y = (a.float().double() for a in synth(20, 8, K, 2, p, gen))
    b.begin("cls_data")
    b.put("X", X)
    b.put("Y", Y)
    for iters in (1, 3):
        for lr in (1.0, 0.5):
            cls_case(b, f"cls_it{iters}_lr{str(lr).replace('.', '')}", X, Y, K, p, iters, lr, gen)
    b.save("dhmm")


if __name__ == "__main__":
    gen_dhmm()
