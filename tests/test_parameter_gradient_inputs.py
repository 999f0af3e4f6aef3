"""CPU tests (no GPU, the oracle alone) of the premises of the central-difference test of the horizon parameter gradient
(tests/test_gpu_rollout_parameter_adjoint.py: test_directional_consistency_with_central_differences_over_with_parameters).

The setting: L = <c_q, q_T> + <c_v, Dq_T>, T = 8, dt = 1e-2, N = 200, the inputs of test_gpu_rollout_adjoint.py's directional test; a random
direction delta on pi, every entry 1 % of its own nominal value times a number uniform in +-1 (_direction); the central
difference of L over the model with pi +- h delta at H = 1 and H / 2 -- the parameters moved by at most 1 % and 0.5 %.  Per sample
    err(h) = |(L(pi + h delta) - L(pi - h delta)) / (2 h) - <gpi, delta>| / scale,
scale = the largest |<gpi_link, delta_link>| over the links (delta is made per link: these are the terms of the inner product).

On the oracle: the oracle chain is built from the perturbed parameters (_oracle_with_parameters) and rolled out with its own forward
dynamics in numpy (test_gpu_rollout.py: _np_rollout over _oracle_fd).  The oracle has no parameter adjoint, so <gpi, delta> is the
extrapolation (4 CD(h / 2) - CD(h)) / 3, exact to O(h^4), and the per-link terms of the scale are central differences along delta
restricted to one link.  With it err(h) = (4 / 3) |CD(h) - CD(h / 2)| and err(h) / err(h / 2) is 4 by construction: what this file pins is
that the samples QUALIFY (err(H) >= 1e-9 scale on at least three quarters of the batch, so that the ratio test on the device has its
samples) and the size of err(H) / scale, which the device test caps with a margin of 2.

Measured (`python tests/test_parameter_gradient_inputs.py`), worst err(H) / scale over the samples and the samples that qualify, of 200:
    chain         err(H) / scale, worst (Euler / RK4)   samples >= 1e-9 scale (Euler / RK4)
    planar_2r     7.839e-05 / 8.097e-05                 200 / 200
    ur10_like     5.840e-05 / 6.196e-05                 200 / 200
    panda_like    4.089e-04 / 3.272e-04                 200 / 200
"""
import numpy as np
import pytest

from _arrays import DIRECTIONAL_DT as DT, DIRECTIONAL_H as H, DIRECTIONAL_N as N, DIRECTIONAL_T as T, INTEGRATORS, _direction, _directional_inputs
from _chains import GRAV, _spec
from _references import ORACLE_WORST, _np_rollout, _oracle_fd

CHAINS = ["planar_2r", "ur10_like", "panda_like"]


def _oracle_with_parameters(name, pi):
    """the oracle chain of `name` with the child links' parameters pi ([m, m c, I about the link origin] per link): mass, centre of mass and
    the inertia about it in the link's axes"""
    from oracle import oracle as orc
    xml, base, tool, inputs = _spec(name)
    spec = orc.urdf_model.load(xml, base, tool, GRAV, inputs)
    for l, link in enumerate(spec.links[1:]):
        m, h = pi[10 * l], pi[10 * l + 1:10 * l + 4]
        if m == 0.0:   # a massless link stays one (its direction is zero)
            assert not pi[10 * l:10 * l + 10].any()
            link.has_inertial, link.mass, link.xyz, link.quat, link.inertia = True, 0.0, [0.0, 0.0, 0.0], (0.0, 0.0, 0.0, 1.0), [0.0] * 6
            continue
        c = h / m
        Io = pi[10 * l + 4:10 * l + 10]
        cc = m * np.array([c[1] ** 2 + c[2] ** 2, -c[0] * c[1], -c[0] * c[2], c[0] ** 2 + c[2] ** 2, -c[1] * c[2], c[0] ** 2 + c[1] ** 2])
        link.has_inertial, link.mass, link.xyz, link.quat, link.inertia = True, float(m), [float(x) for x in c], (0.0, 0.0, 0.0, 1.0), [float(x) for x in Io - cc]
    real = orc.urdf_model.load
    orc.urdf_model.load = lambda *a, **k: spec
    try:
        return orc.OracleChain(xml, base, tool, GRAV, input_joint_names=inputs)
    finally:
        orc.urdf_model.load = real


def _pi_of(name):
    from rosdyn_amd import Chain
    xml, base, tool, inputs = _spec(name)
    chain = Chain(xml, base, tool, GRAV)
    return chain.getNominalParameters()


def measure(name, integrator):
    """(err(H) / scale per sample, on the oracle)"""
    pi = _pi_of(name)
    delta = _direction(pi)
    ref = _oracle_with_parameters(name, pi)
    q0, dq0, tau, cq, cv = _directional_inputs(name, ref.n, N, T)[:5]

    def loss(p):
        qe, ve = _np_rollout(_oracle_fd(_oracle_with_parameters(name, p)), q0, dq0, tau, DT, T, integrator)
        return (cq * qe).sum(axis=1) + (cv * ve).sum(axis=1)

    cd = lambda d, h: (loss(pi + h * d) - loss(pi - h * d)) / (2.0 * h)
    big, small = cd(delta, H), cd(delta, 0.5 * H)
    err = np.abs(big - (4.0 * small - big) / 3.0)
    terms = []
    for l in range(len(pi) // 10):
        d = np.zeros_like(delta)
        d[10 * l:10 * l + 10] = delta[10 * l:10 * l + 10]
        terms.append(np.abs(cd(d, 0.5 * H)))
    return err / np.max(terms, axis=0)


def test_the_round_trip_through_a_link_description_returns_the_parameters():
    for name in CHAINS:
        pi = _pi_of(name)
        moved = pi + _direction(pi)
        ref = _oracle_with_parameters(name, moved)
        q, dq, ddq = (np.random.default_rng(7 + i).uniform(-1.0, 1.0, (5, ref.n)) for i in range(3))
        Y, tau = ref.regressor(q, dq, ddq), ref.joint_torque(q, dq, ddq)
        assert (np.abs(Y @ moved - tau) <= 1e-12 * (np.abs(Y) @ np.abs(moved))).all(), name


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("name", CHAINS)
def test_the_samples_qualify_and_the_error_is_what_was_recorded(name, integrator):
    r = measure(name, integrator)
    qualify = int((r >= 1e-9).sum())
    recorded = ORACLE_WORST[name][INTEGRATORS.index(integrator)]
    print("%s %s: worst err(H) / scale %.3g (recorded %.3g), %d of %d samples qualify" % (name, integrator, r.max(), recorded, qualify, N))
    assert qualify >= 3 * N // 4, qualify
    assert abs(r.max() / recorded - 1.0) <= 0.01, (float(r.max()), recorded)


if __name__ == "__main__":
    for name in CHAINS:
        out = []
        for integrator in INTEGRATORS:
            r = measure(name, integrator)
            out.append((r.max(), int((r >= 1e-9).sum())))
        print("    %-12s %.3e / %.3e   %d / %d" % (name, out[0][0], out[1][0], out[0][1], out[1][1]))
