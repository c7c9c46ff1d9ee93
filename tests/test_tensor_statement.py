"""
The tensor algorithm of tests/_tensor_form.py (d corrector solves + cross integrals of the correctors) against the scalar
oracle driver: xi' Sigma xi is what oracle.checkerboard_homogenization(xi=xi) returns.  These tests hold the formula the device
tests (tests/test_gpu_tensor.py) rely on; they need no GPU.

Bound 1e-10, from the stopping rule: a cycle loop that stops at |D_i - D_{i-1}| < tol while the increments contract by at most
0.86 per cycle is within tol * 0.86 / 0.14 of its limit; with tol = 1e-12 / 1e-13 that leaves room for up
to four such terms per entry, two outer steps and the factor 2^k.  Measured: 5.3e-14 (2D), 3.5e-13 (3D).
"""
import numpy as np
import pytest

from _tensor_form import checkerboard_homogenization_tensor, polarised

pytestmark = pytest.mark.slow

BOUND = 1e-10


def test_2d_with_a_domain_shrink_matches_the_scalar_runs(oracle):
    O = oracle
    kw = dict(n=5, dim=2, refinements=1, tolerance=1e-12, seed=3)
    Sigma, hist = checkerboard_homogenization_tensor(**kw)
    assert {h[0] for h in hist} == {0, 1}                    # a domain shrink is included
    assert {(h[0], h[1]) for h in hist} == {(k, d) for k in (0, 1) for d in (0, 1)}
    assert np.array_equal(Sigma, Sigma.T)
    s = 1.0 / np.sqrt(2.0)
    for xi in ((1.0, 0.0), (0.0, 1.0), (s, s), (s, -s)):
        xi = np.array(xi)
        want, hist_s = O.checkerboard_homogenization(xi=xi, **kw)
        assert {h[0] for h in hist_s} == {0, 1}
        got = float(xi @ Sigma @ xi)
        print(f"xi = {xi}: tensor {got:.15f}  scalar {want:.15f}  diff {got - want:.2e}")
        assert abs(got - want) <= BOUND, (xi, got, want)


def test_3d_all_six_entries_match_the_polarisation_of_six_scalar_runs(oracle):
    O = oracle
    kw = dict(n=0, dim=3, refinements=1, tolerance=1e-13, seed=3)
    Sigma, hist = checkerboard_homogenization_tensor(**kw)
    assert {h[0] for h in hist} == {0}
    want = polarised(lambda xi: O.checkerboard_homogenization(xi=xi, **kw)[0], 3)
    print("tensor\n", Sigma, "\npolarised\n", want, "\nlargest difference", np.abs(Sigma - want).max())
    assert np.array_equal(Sigma, Sigma.T)
    assert np.abs(Sigma - want).max() <= BOUND, (Sigma, want)
