"""GPU parity of the driven HMM: the K16 forward-backward kernel against outputs of the reference
(tests/golden/dhmm.npz) and, on larger seeded inputs, against the CPU restatement tests/dhmm_oracle.py; the dHMM class
(MNLR gate + NIW emissions + K16) against the reference's raw_update."""
import pytest
import torch

from tests import dhmm_oracle
from tests.helpers import TOL32, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"

FB_CASES = ["fb_k4_T100_S199", "fb_k25", "fb_k2_T2", "fb_k9_T1", "fb_k5_ptemp", "fb_k3_b2", "fb_k6_forbidden", "fb_k5_peaked"]


def run(obs, tr, init, batch, ptemp, dtype):
    from pyvbmp_amd import ops
    return ops.dhmm_forward_backward(obs.to(DEV, dtype), tr.to(DEV, dtype), init.to(DEV, dtype), batch, ptemp)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", FB_CASES)
def test_dhmm_forward_backward_golden(golden, case, dtype):
    c = golden("dhmm")[case]
    batch = tuple(int(v) for v in c["batch_shape"])
    obs, tr, init = dhmm_oracle.golden_inputs(c)
    p, SEzz, SEz0, logZ = run(obs, tr, init, batch, float(c["ptemp"]), dtype)
    tol = 1e-10 if dtype == torch.float64 else TOL32
    (p_got, p_ref), (zz_got, zz_ref) = dhmm_oracle.golden_outputs(c, p, SEzz)
    assert_close(p_got, p_ref, tol, what="p")
    assert_close(zz_got, zz_ref, tol, what="SEzz")
    assert_close(SEz0, c["SEz0"], tol, what="SEz0")
    assert_close(logZ, c["logZ"], tol, what="logZ")
    if "p_head" in c:
        # the fixture keeps p and SEzz of the first series only: all series against the restatement, which
        # tests/test_dhmm_host.py pins to the reference on that head
        rp, rzz, _, _ = dhmm_oracle.forward_backward(obs.to(dtype).double(), tr.to(dtype).double(), init.to(dtype).double(),
                                                     float(c["ptemp"]))
        assert_close(p, rp, tol, what="p (all series)")
        assert_close(SEzz, rzz, tol, what="SEzz (all series)")


def random_case(K, T, S, batch, g, obs_scale=2.0, tr_scale=1.5, keep=None):
    lead = (S,) + tuple(batch)
    obs = obs_scale * torch.randn((T,) + lead + (K,), generator=g, dtype=torch.float64)
    tr = torch.log_softmax(tr_scale * torch.randn((T,) + lead + (K, K), generator=g, dtype=torch.float64), -1)
    if keep is not None:
        mask = torch.rand((T,) + lead + (K, K), generator=g) < keep
        mask |= torch.eye(K, dtype=torch.bool).roll(1, -1)  # a cycle: every state reachable, every state has a successor
        tr = torch.where(mask, tr, torch.full_like(tr, -float("inf")))
    init = torch.log_softmax(torch.randn(tuple(batch) + (K,), generator=g, dtype=torch.float64), -1)
    return obs, tr, init


def check_vs_oracle(obs, tr, init, batch, ptemp, dtype, tol):
    p, SEzz, SEz0, logZ = run(obs, tr, init, batch, ptemp, dtype)
    # the oracle sees the operands the kernel saw
    obs, tr, init = obs.to(dtype).double(), tr.to(dtype).double(), init.to(dtype).double()
    rp, rzz, rz0, rlz = dhmm_oracle.forward_backward(obs, tr, init, ptemp)
    assert_close(p, rp, tol, what="p")
    assert_close(SEzz, rzz, tol, what="SEzz")
    assert_close(SEz0, rz0, tol, what="SEz0")
    assert_close(logZ, rlz, tol, what="logZ")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,T,S,batch,ptemp,keep", [(2, 500, 300, (), 1.0, None), (3, 200, 150, (2,), 1.7, None),
                                                    (8, 300, 200, (3,), 1.0, 0.5), (25, 120, 60, (2,), 0.6, None),
                                                    (33, 60, 40, (), 1.0, 0.3), (64, 40, 24, (2,), 2.0, None)])
def test_dhmm_forward_backward_vs_oracle(K, T, S, batch, ptemp, keep, dtype):
    """every lane-group width (Kp = 2 .. 64) incl. padded ones, several hundred chains, NB > 1, ptemp != 1, forbidden moves"""
    g = torch.Generator().manual_seed(K * 131 + T)
    obs, tr, init = random_case(K, T, S, batch, g, keep=keep)
    check_vs_oracle(obs, tr, init, batch, ptemp, dtype, 1e-10 if dtype == torch.float64 else TOL32 * 5)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K,T,S,obs_scale,tr_scale,keep", [(5, 80, 40, 400.0, 40.0, None), (8, 60, 64, 1500.0, 5.0, 0.3),
                                                           (25, 30, 8, 250.0, 60.0, 0.2)])
def test_dhmm_extreme_logits(K, T, S, obs_scale, tr_scale, keep, dtype):
    """logits spread over hundreds to thousands of nats: row sums of the pair weights underflow and the kernel redoes those
    rows in log space"""
    g = torch.Generator().manual_seed(K * 17 + T)
    obs, tr, init = random_case(K, T, S, (), g, obs_scale=obs_scale, tr_scale=tr_scale, keep=keep)
    # fp32: the running log-likelihood reaches ~1e5 here, where one fp32 ulp is 8e-3 -- the message differences that decide
    # an ambiguous state carry that absolute error whatever the recursion (as for K11's extreme-logit test)
    check_vs_oracle(obs, tr, init, (), 1.0, dtype, 1e-10 if dtype == torch.float64 else 5e-3)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dhmm_unreachable_column_is_nan_as_in_the_reference(dtype):
    """a target state no source reaches at some step: the reference's log-sum-exp over -inf is NaN, and the whole chain
    follows; the other chains are untouched"""
    g = torch.Generator().manual_seed(5)
    obs, tr, init = random_case(4, 12, 3, (), g)
    tr[6, 1, :, 2] = -float("inf")
    p, SEzz, SEz0, logZ = run(obs, tr, init, (), 1.0, dtype)
    rp, rzz, rz0, rlz = dhmm_oracle.forward_backward(obs.to(dtype).double(), tr.to(dtype).double(), init.to(dtype).double())
    assert torch.isnan(rlz[1]) and torch.isfinite(rlz[0])
    tol = 1e-10 if dtype == torch.float64 else TOL32 * 5
    for a, b in ((p, rp), (SEzz, rzz), (SEz0, rz0), (logZ, rlz)):
        assert_close(a, b, tol)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dhmm_full_size_properties(dtype):
    """T = 1000, C = 4096, K = 8: every SEzz[t] and every p row sums to 1; every 257th chain equals the restatement"""
    K, T, C = 8, 1000, 4096
    g = torch.Generator().manual_seed(8)
    obs = (2.0 * torch.randn(T, C, K, generator=g, dtype=torch.float64)).to(dtype)
    tr = torch.log_softmax(1.5 * torch.randn(T, C, K, K, generator=g, dtype=torch.float64), -1).to(dtype)
    init = torch.log_softmax(torch.randn(K, generator=g, dtype=torch.float64), -1).to(dtype)
    p, SEzz, SEz0, logZ = run(obs, tr, init, (), 1.0, dtype)
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert (SEzz.sum((-1, -2)) - 1).abs().max().item() < tol
    assert (p.sum(-1) - 1).abs().max().item() < tol
    assert (SEz0.sum(-1) - 1).abs().max().item() < tol
    idx = torch.arange(0, C, 257)
    rp, rzz, rz0, rlz = dhmm_oracle.forward_backward(obs[:, idx].double(), tr[:, idx].double(), init.double())
    tol = 1e-10 if dtype == torch.float64 else TOL32 * 5
    assert_close(p[:, idx], rp, tol, what="p")
    assert_close(SEzz[:, idx], rzz, tol, what="SEzz")
    assert_close(SEz0[idx], rz0, tol, what="SEz0")
    assert_close(logZ[idx], rlz, tol, what="logZ")


def make_model(c, dtype=torch.float64):
    from pyvbmp_amd.dists import NormalInverseWishart
    from pyvbmp_amd.models import dHMM
    K, p = int(c["K"]), int(c["xdim"])
    m = dHMM(NormalInverseWishart((2,), (K,), device=DEV, dtype=dtype), p)
    # the reference draws the initial NIW mean and the gate's coefficient posterior (incl. its ARD Gamma factor) at random:
    # replay the stored draws
    m.obs_dist.mu = c["init_niw_mu"].to(DEV, dtype)
    q = m.transition.beta
    for f in ("mu", "invSigma", "invSigmamu", "Sigma", "logdetinvSigma"):
        setattr(q, f, c["init_beta_" + f].to(DEV, dtype))
    q.alpha.alpha = c["init_beta_alpha"].to(DEV, dtype)
    q.alpha.beta = c["init_beta_beta"].to(DEV, dtype)
    return m


@pytest.mark.parametrize("case", ["cls_it1_lr10", "cls_it1_lr05", "cls_it3_lr10", "cls_it3_lr05"])
def test_dhmm_class_golden(golden, case):
    """dHMM.raw_update (K16 + MNLR gate with a (K,) batch + NIW emissions + Dirichlet initial) against the reference"""
    c, data = golden("dhmm")[case], golden("dhmm")["cls_data"]
    m = make_model(c)
    m.raw_update(data["X"].to(DEV), data["Y"].to(DEV), iters=int(c["iters"]), lr=float(c["lr"]))
    tol = 1e-10
    got = {"niw_lambda_mu": m.obs_dist.lambda_mu, "niw_mu": m.obs_dist.mu, "niw_invU": m.obs_dist.invU.invU,
           "niw_nu": m.obs_dist.invU.nu, "beta_mu": m.transition.beta.mu, "beta_invSigma": m.transition.beta.invSigma,
           "initial_alpha": m.initial.alpha, "p": m.p, "SEzz": m.SEzz, "SEz0": m.SEz0, "NA": m.NA, "logZ": m.logZ,
           "sumlogZ": m.sumlogZ, "KLqprior": m.KLqprior(), "ELBO": m.ELBO()}
    for k, v in got.items():
        assert_close(v, c[k], tol, what=k)


def test_dhmm_beyond_the_kernel_limit_raises():
    """more than VBMP_DHMM_MAX_K = 64 states: a VbmpHipError naming the limit at construction (no host-loop fallback)"""
    from pyvbmp_amd import _lib
    from pyvbmp_amd.dists import NormalInverseWishart
    from pyvbmp_amd.models import dHMM
    with pytest.raises(_lib.VbmpHipError, match="VBMP_DHMM_MAX_K"):
        dHMM(NormalInverseWishart((2,), (65,), device=DEV, dtype=torch.float64), 3)
    with pytest.raises(_lib.VbmpHipError):
        from pyvbmp_amd import ops
        ops.dhmm_forward_backward(torch.zeros(3, 2, 4, dtype=torch.float64), torch.zeros(3, 2, 4, 4, dtype=torch.float64),
                                  torch.zeros(4, dtype=torch.float64), ())
