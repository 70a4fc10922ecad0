"""Driven HMM without a GPU: the K16 entry points are exported and validate their arguments on the host, and the CPU
restatement tests/dhmm_oracle.py reproduces every kernel-level output of the reference (tests/golden/dhmm.npz)."""
import ctypes

import pytest

from tests import dhmm_oracle
from tests.helpers import assert_close

FB_CASES = ["fb_k4_T100_S199", "fb_k25", "fb_k2_T2", "fb_k9_T1", "fb_k5_ptemp", "fb_k3_b2", "fb_k6_forbidden", "fb_k5_peaked"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pyvbmp_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_dhmm_entry_points_reject_bad_arguments_without_a_gpu(lib, suf):
    from pyvbmp_amd import _lib
    fn = getattr(lib, "vbmp_dhmm_forward_backward_" + suf)
    cT = _lib.DTYPES[suf][1]
    some, null = ctypes.c_void_p(64), ctypes.c_void_p(0)
    outs = [some] * 4

    def call(ptrs, T, C, NB, K):
        return fn(*ptrs[:3], T, C, NB, K, cT(1.0), *ptrs[3:], null)
    assert call([some] * 3 + outs, 5, 7, 1, 65) == -1      # K beyond VBMP_DHMM_MAX_K
    assert call([some] * 3 + outs, 5, 7, 1, 0) == -1       # K < 1
    assert call([null] + [some] * 2 + outs, 5, 7, 1, 4) == -1
    assert call([some] * 3 + [some, null, some, some], 5, 7, 1, 4) == -1
    assert call([some] * 3 + outs, -1, 7, 1, 4) == -1
    assert call([some] * 3 + outs, 5, -7, 1, 4) == -1
    assert call([some] * 3 + outs, 5, 7, 0, 4) == -1       # no initial distribution
    assert call([null] * 7, 5, 0, 1, 4) == 0               # empty work: nothing to do
    assert call([null] * 7, 0, 7, 1, 4) == 0


def test_dhmm_limit_matches_the_header():
    import os
    import re
    from pyvbmp_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vbmp_hip.h")).read()
    assert int(re.search(r"#define VBMP_DHMM_MAX_K (\d+)", hdr).group(1)) == _lib.DHMM_MAX_K


@pytest.mark.parametrize("case", FB_CASES)
def test_dhmm_oracle_reproduces_the_reference(golden, case):
    c = golden("dhmm")[case]
    obs, tr, init = dhmm_oracle.golden_inputs(c)
    p, SEzz, SEz0, logZ = dhmm_oracle.forward_backward(obs, tr, init, float(c["ptemp"]))
    (p, p_ref), (SEzz, zz_ref) = dhmm_oracle.golden_outputs(c, p, SEzz)
    assert_close(p, p_ref, 1e-10, what="p")
    assert_close(SEzz, zz_ref, 1e-10, what="SEzz")
    assert_close(SEz0, c["SEz0"], 1e-10, what="SEz0")
    assert_close(logZ, c["logZ"], 1e-10, what="logZ")
