"""CPU tests (no GPU) of rdyn_chain_with_parameters / Chain.withParameters: a chain with other inertial parameters, equal to a clone in
everything else.  The parameters are stored as given (include/rdyn.h), so what comes back is compared bit for bit where the issue's bound
is 1e-14 max |pi'_link|; the reduced companion's merged parameters are sums of X-images, bound 1e-13 of their terms."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import FIXTURES

GRAV = (0.0, 0.0, -9.806)
CHAINS = {
    "ur10_like": ("ur10_like.urdf", "base_link", "tool0"),
    "ur10_public": ("ur10_public.urdf", "base_link", "tool0"),
    "mixed_joints": ("mixed_joints.urdf", "world", "tip"),
    "ur10_public_long": ("ur10_public_long.urdf", "base_link", "tcp"),
}


def _chain(name):
    from rosdyn_amd import Chain
    f, base, tool = CHAINS[name]
    return Chain(os.path.join(FIXTURES, f), base, tool, GRAV)


def _perturbed(pi, seed=5):
    return pi * (1.0 + 0.1 * np.random.default_rng(seed).uniform(-1.0, 1.0, pi.shape))


def _link_parameters(chain, i):
    from rosdyn_amd._lib import check, lib
    pi, mass, cog = np.zeros(10), C.c_double(), np.zeros(3)
    dp = C.POINTER(C.c_double)
    check(lib().rdyn_chain_link_parameters(chain._h, i, pi.ctypes.data_as(dp), C.byref(mass), cog.ctypes.data_as(dp)))
    return pi, mass.value, cog


def _constants(chain, i):
    from rosdyn_amd._lib import check, lib
    out = [np.zeros(9), np.zeros(3), np.zeros(3), np.zeros(5)]
    check(lib().rdyn_chain_joint_constants(chain._h, i, *[x.ctypes.data_as(C.POINTER(C.c_double)) for x in out]))
    return np.concatenate(out)


@pytest.mark.parametrize("name", list(CHAINS))
def test_the_parameters_come_back_and_everything_else_is_the_clones(name):
    chain = _chain(name)
    pi0 = chain.getNominalParameters()
    pi1 = _perturbed(pi0)
    other = chain.withParameters(pi1)
    got = other.getNominalParameters()
    for l in range(chain.getJointsNumber()):
        sl = slice(10 * l, 10 * l + 10)
        assert np.abs(got[sl] - pi1[sl]).max() <= 1e-14 * np.abs(pi1[sl]).max()
        p, mass, cog = _link_parameters(other, l + 1)
        assert np.array_equal(p, got[sl]) and mass == pi1[10 * l]
        if mass != 0.0:
            assert np.abs(cog * mass - pi1[10 * l + 1:10 * l + 4]).max() <= 1e-14 * np.abs(pi1[sl]).max()
    assert np.array_equal(got, pi1)  # stored as given
    # the base link keeps its inertial, the original chain everything
    assert all(np.array_equal(a, b) for a, b in zip(_link_parameters(other, 0)[::2], _link_parameters(chain, 0)[::2]))
    assert np.array_equal(chain.getNominalParameters(), pi0)
    for what in ("getLinksName", "getJointsName", "getActiveJointsName", "getMoveableJointNames", "getJointTypes"):
        assert getattr(other, what)() == getattr(chain, what)()
    for what in ("getGravity", "getQMax", "getQMin", "getDQMax", "getDDQMax", "getTauMax"):
        assert np.array_equal(getattr(other, what)(), getattr(chain, what)())
    for j in range(chain.getJointsNumber()):
        assert np.array_equal(_constants(other, j), _constants(chain, j))
    # a clone of the new chain, and a chain made from it again, carry the parameters on
    assert np.array_equal(other.clone().getNominalParameters(), pi1)
    assert np.array_equal(other.withParameters(pi0).getNominalParameters(), pi0)


def test_a_permuted_input_selection_is_preserved_and_can_still_change():
    chain = _chain("ur10_like")
    names = chain.getActiveJointsName()
    order = [names[i] for i in (4, 0, 5, 2)]
    assert chain.setInputJointsName(order)
    pi1 = _perturbed(chain.getNominalParameters())
    other = chain.withParameters(pi1)
    assert other.getActiveJointsName() == order and np.array_equal(other.getQMax(), chain.getQMax())
    # independent: re-configuring one does not touch the other, and the parameters survive the re-configuration
    assert other.setInputJointsName(names)
    assert chain.getActiveJointsName() == order and other.getActiveJointsName() == names
    assert np.array_equal(other.getNominalParameters(), pi1)


@pytest.mark.parametrize("name", ["ur10_public", "ur10_public_long"])
def test_the_reduced_companion_is_rebuilt_from_the_new_parameters(name):
    chain = _chain(name)
    pi1 = _perturbed(chain.getNominalParameters(), seed=8)
    other = chain.withParameters(pi1)
    body0, X0, _ = chain.getBodyReduction()
    body, X, pi_body = other.getBodyReduction()
    assert np.array_equal(body, body0) and np.array_equal(X, X0)
    bodies = [j for j in range(chain.getJointsNumber()) if body[j] == j]
    assert len(bodies) == len(pi_body)
    for r, b in enumerate(bodies):
        terms = np.array([X[f] @ pi1[10 * f:10 * f + 10] for f in range(len(body)) if body[f] == b])
        mags = np.array([np.abs(X[f]) @ np.abs(pi1[10 * f:10 * f + 10]) for f in range(len(body)) if body[f] == b])
        assert (np.abs(pi_body[r] - terms.sum(axis=0)) <= 1e-13 * mags.sum(axis=0)).all()
    assert not np.array_equal(pi_body, chain.getBodyReduction()[2])


def test_a_massless_link_with_inertia_is_kept_and_what_is_not_finite_is_refused():
    from rosdyn_amd._lib import lib
    chain = _chain("ur10_like")
    pi = chain.getNominalParameters()
    odd = pi.copy()
    odd[10:20] = [0.0, 0.1, -0.2, 0.3, 1.0, 0.01, 0.02, 2.0, 0.03, 3.0]   # no mass, a first moment and an inertia
    other = chain.withParameters(odd)
    assert np.array_equal(other.getNominalParameters(), odd)
    p, mass, cog = _link_parameters(other, 2)
    assert np.array_equal(p, odd[10:20]) and mass == 0.0 and np.array_equal(cog, np.zeros(3))
    for value in (np.nan, np.inf, -np.inf):
        bad = pi.copy()
        bad[23] = value
        with pytest.raises(ValueError) as e:
            chain.withParameters(bad)
        assert chain.getLinksName()[3] in str(e.value)
    with pytest.raises(ValueError):
        chain.withParameters(pi[:-1])
    h = C.c_void_p()
    dp = C.POINTER(C.c_double)
    assert lib().rdyn_chain_with_parameters(None, pi.ctypes.data_as(dp), C.byref(h)) == 1
    assert lib().rdyn_chain_with_parameters(chain._h, None, C.byref(h)) == 1
    assert lib().rdyn_chain_with_parameters(chain._h, pi.ctypes.data_as(dp), None) == 1
