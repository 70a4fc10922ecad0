"""Driven (input-output) hidden Markov model: p(z_t | z_{t-1}, x_t) is a multinomial logistic regression on the input
x_t, p(y_t | z_t) the observation node (surface of the reference's models/dHMM.py:10-137).

The transition matrix changes at every step, so the forward-backward recursion (:42-78) needs a K x K matrix per
(step, series) and returns the pair posterior per step -- the gate's M-step regresses SEzz[t] on x_t.  The recursion is
ONE persistent HIP launch (K16, csrc/k_dhmm.hip); the transition logits come from the gate's log_predict, the emission
terms and updates from the observation node's kernels, the gate update from MultiNomialLogisticRegression.raw_update.
"""
import torch

from .. import ops
from ..dists.Dirichlet import Dirichlet
from ..transforms.MultiNomialLogisticRegression import MultiNomialLogisticRegression


class dHMM():
    def __init__(self, obs_dist, p, transition_mask=None, ptemp=1.0):
        self.obs_dist = obs_dist
        self.device, self.dtype = obs_dist.device, obs_dist.dtype
        n = obs_dist.batch_shape[-1]
        if n > ops.L.DHMM_MAX_K:
            # a host loop over time in torch ops would be the silent slow path this package does not have
            raise ops.L.VbmpHipError(f"dHMM with {n} states: the forward-backward kernel (K16) holds a step's transition "
                                     f"column in registers and serves up to VBMP_DHMM_MAX_K = {ops.L.DHMM_MAX_K} states")
        self.hidden_dim = n
        self.event_dim = 1
        self.event_shape = (n,)
        self.batch_shape = tuple(obs_dist.batch_shape[:-1])
        self.batch_dim = len(self.batch_shape)
        self.ptemp = ptemp
        self.transition_mask = transition_mask  # accepted and not used, as in the reference
        kw = {"device": self.device, "dtype": self.dtype}
        self.transition = MultiNomialLogisticRegression(n, p, batch_shape=self.batch_shape + (n,), pad_X=True, **kw)
        self.initial = Dirichlet((n,), self.batch_shape, **kw)
        self.initial.alpha = self.initial.alpha_0
        self.sumlogZ = -torch.inf
        self.p = None

    def to_event(self, n):
        if n < 1:
            return self
        self.event_dim = self.event_dim + n
        self.batch_dim = self.batch_dim - n
        self.event_shape = self.batch_shape[-n:] + self.event_shape
        self.batch_shape = self.batch_shape[:-n]
        return self

    # single steps of the recursion (ref :34-38), for callers that step by hand; the sweep itself is K16
    def forward_step(self, logits, observation_logits, transition_logits):
        return torch.logsumexp(logits.unsqueeze(-1) + observation_logits.unsqueeze(-2) + transition_logits, -2)

    def backward_step(self, logits, observation_logits, transition_logits):
        return torch.logsumexp(logits.unsqueeze(-2) + observation_logits.unsqueeze(-2) + transition_logits, -1)

    def forward_backward_loop(self, fw_logits, transition_logits):
        """Time first: fw_logits (T,)+sample+batch+(K,) observation logits, transition_logits broadcastable to
        (T,)+sample+batch+(K,K).  Sets self.p; returns SEzz (per step, time NOT integrated out), SEz0, logZ.  One K16
        launch (ref :42-78)."""
        self.p, SEzz, SEz0, logZ = ops.dhmm_forward_backward(fw_logits, transition_logits, self.initial.loggeomean(),
                                                             self.batch_shape, self.ptemp)
        return SEzz, SEz0, logZ

    def assignment_pr(self):
        return self.p

    def assignment(self):
        return self.p.argmax(-1)

    def obs_logits(self, Y):
        return self.obs_dist.Elog_like(Y)

    def transition_logits(self, X):
        return self.transition.log_predict(X)

    def raw_update_states(self, X, Y):
        """state posteriors (self.p), per-step pair statistics self.SEzz, self.SEz0, self.NA, self.logZ (per sample) and
        self.sumlogZ (ref :95-108)"""
        SEzz, SEz0, logZ = self.forward_backward_loop(self.obs_logits(Y), self.transition_logits(X))
        NA = self.p.sum(0)
        self.logZ = logZ
        sd = tuple(range(NA.ndim - self.batch_dim - self.event_dim))
        if sd:
            NA, SEz0, logZ = NA.sum(sd), SEz0.sum(sd), logZ.sum(sd)
        self.SEzz = SEzz
        self.SEz0 = SEz0
        self.NA = NA
        self.sumlogZ = logZ

    def raw_update_markov_parms(self, X, lr=1.0):
        self.transition.raw_update(X, self.SEzz, iters=4, lr=lr)
        self.initial.ss_update(self.SEz0, lr)

    def raw_update_obs_parms(self, Y, lr=1.0):
        self.obs_dist.raw_update(Y, self.p, lr)

    def raw_update(self, X, Y, iters=1, lr=1.0, verbose=False):
        """X: (T,)+sample+batch+(p,) inputs, Y: (T,)+sample+batch+obs event observations (ref :120-135)"""
        Y = Y.unsqueeze(-2)
        X = X.unsqueeze(-2)
        ELBO = torch.tensor(-torch.inf, device=self.device, dtype=self.dtype)
        for i in range(iters):
            ELBO_last = ELBO
            self.raw_update_states(X, Y)
            self.KLqprior_last = self.KLqprior()
            self.raw_update_markov_parms(X, lr)
            self.raw_update_obs_parms(Y, lr)
            ELBO = self.ELBO().sum()
            if verbose:
                print('Percent Change in ELBO = %f' % ((ELBO - ELBO_last) / ELBO_last.abs() * 100))

    def KLqprior(self):
        # the gate's KL stays per from-state, so the sum has shape batch + (K,) as in the reference (:137-141)
        KL = self.obs_dist.KLqprior().sum(-1) + self.transition.KLqprior() + self.initial.KLqprior()
        for i in range(self.event_dim - 1):
            KL = KL.sum(-1)
        return KL

    def ELBO(self):
        return self.sumlogZ - self.KLqprior()
