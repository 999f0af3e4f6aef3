"""Test support: friction and spring component lists, their ComponentSet, and the closed-form slopes pinned to the oracle."""
import numpy as np

from _arrays import TAU_SCALE


FRICTION1, FRICTION2, SPRING = 0, 1, 2
MIN_VELOCITY, MAX_VELOCITY = 0.3, 0.8   # Dq uniform in +-1: about 30 % of the entries in the band, 20 % saturated


def _specs(n):
    """(type, joint, min_velocity, max_velocity, parameters) in list order: two friction components and a spring on joint 0, a FRICTION2 on
    the last input joint, a spring on joint 1"""
    specs = [(FRICTION1, 0, MIN_VELOCITY, MAX_VELOCITY, (2.0, 1.5, 0.0)),
             (FRICTION2, n - 1, MIN_VELOCITY, MAX_VELOCITY, (1.0, 0.8, -0.6)),
             (SPRING, 1, 0.0, 0.0, (3.0, -0.4, 0.0)),
             (SPRING, 0, 0.0, 0.0, (-1.5, 0.3, 0.0)),
             (FRICTION2, 0, MIN_VELOCITY, MAX_VELOCITY, (0.5, 0.2, 0.4))]
    return specs


def _set(specs, n):
    from rosdyn_amd.components import ComponentSet
    return ComponentSet([dict(type=t, joint=j, min_velocity=lo, max_velocity=hi, parameters=list(p)) for t, j, lo, hi, p in specs], n)


def _slopes(specs, q, dq):
    """closed form: (d tau_c / d q, d tau_c / d dq), each (N, n) -- the diagonals"""
    sq, sv = np.zeros_like(q), np.zeros_like(dq)
    for ty, j, lo, hi, p in specs:
        if ty == SPRING:
            sq[:, j] += p[0]
            continue
        x = dq[:, j]
        w = np.clip(x, -hi, hi)
        dw = (np.abs(x) < hi).astype(float)
        band = np.abs(w) < lo
        sg = np.where(band, w / lo, np.sign(w))
        dsg = np.where(band, 1.0 / lo, 0.0)
        s = p[0] * dsg + p[1]
        if ty == FRICTION2:
            s = s + p[2] * (2.0 * w * sg + w * w * dsg)
        sv[:, j] += dw * s
    return sq, sv


def _pin_the_closed_form_to_the_oracle(specs, n, q, dq):
    from oracle.oracle import components_regressor
    h = 2.0 ** -10
    tau_c = lambda qq, vv: components_regressor(specs, n, qq, vv)[1]
    stencil = lambda f: (-f(2 * h) + 8.0 * f(h) - 8.0 * f(-h) + f(-2 * h)) / (12.0 * h)
    num_q = stencil(lambda d: tau_c(q + d, dq))
    num_v = stencil(lambda d: tau_c(q, dq + d))
    sq, sv = _slopes(specs, q, dq)
    big = np.abs(tau_c(q, dq)).max()
    assert (np.abs(num_q - sq) <= 1e-11 * (np.abs(sq) + big / h)).all()
    far = np.ones_like(dq, dtype=bool)
    for kink in (-MAX_VELOCITY, -MIN_VELOCITY, MIN_VELOCITY, MAX_VELOCITY):
        far &= np.abs(dq - kink) >= 2.0 ** -8
    left_out = 1.0 - far.mean()
    err = np.abs(num_v - sv) / (np.abs(sv) + big / h)
    print("closed form against the oracle's stencil: worst ratio %.3g (bound 1e-11), %.2f %% of the entries left out (cap 5 %%)"
          % (err[far].max(), 100.0 * left_out))
    assert left_out <= 0.05
    assert (err[far] <= 1e-11).all()


COMPONENT_SCALE = dict(TAU_SCALE, ur10_permuted=TAU_SCALE["ur10_like"])

ROLLOUT_MIN_VELOCITY, ROLLOUT_MAX_VELOCITY = 0.05, 0.8   # |dq| <= 1: a few percent of the joints inside the linear band, the velocity saturation is hit

# Coulomb parameters shrunk per chain until the oracle alone keeps dev of MULTI_STEP_C below 1e-9 (the in-band slope coulomb / min_velocity
# against the light last links of these chains); 1 where not listed
COULOMB = {"ur10_like": 0.3, "panda_like": 0.3, "mixed_joints": 0.3, "ur10_public_long": 0.3, "rev14": 0.3}


def _scaled_specs(name, n, coulomb=None):
    """(type, joint, min_velocity, max_velocity, parameters) in list order: a FRICTION1 and, later in the list, a SPRING on joint 0 (two
    components share a joint, list order matters), a FRICTION2 on the last input joint, a SPRING on joint 1; with n >= 4 the joints
    2 .. n - 2 have no component.  Parameters of order 1 times the chain's torque scale."""
    s = COMPONENT_SCALE[name]
    coulomb = COULOMB.get(name, 1.0) if coulomb is None else coulomb
    specs = [(FRICTION1, 0, ROLLOUT_MIN_VELOCITY, ROLLOUT_MAX_VELOCITY, (0.9 * coulomb * s, 0.7 * s, 0.0))]
    if n >= 2:
        specs.append((FRICTION2, n - 1, ROLLOUT_MIN_VELOCITY, ROLLOUT_MAX_VELOCITY, (0.8 * coulomb * s, 0.5 * s, -0.6 * s)))
    if n >= 3:
        specs.append((SPRING, 1, 0.0, 0.0, (1.1 * s, -0.4 * s, 0.0)))
    specs.append((SPRING, 0, 0.0, 0.0, (-0.8 * s, 0.3 * s, 0.0)))
    return specs


def _named_components(name, n):
    return _set(_scaled_specs(name if name in TAU_SCALE or name == "ur10_permuted" else "ur10_like", n), n)


AUTOGRAD_MIN_VELOCITY, AUTOGRAD_MAX_VELOCITY = 0.05, 1000.0


def _autograd_components(n):
    """friction on the first two joints (band +-0.05, saturation far away), a spring on joint 0"""
    from rosdyn_amd.components import ComponentSet
    return ComponentSet([dict(type=FRICTION1, joint=0, min_velocity=AUTOGRAD_MIN_VELOCITY, max_velocity=AUTOGRAD_MAX_VELOCITY, parameters=[0.3, 0.2, 0.0]),
                         dict(type=FRICTION1, joint=1, min_velocity=AUTOGRAD_MIN_VELOCITY, max_velocity=AUTOGRAD_MAX_VELOCITY, parameters=[0.1, 0.05, 0.0]),
                         dict(type=SPRING, joint=0, min_velocity=0.0, max_velocity=0.0, parameters=[2.0, -0.1, 0.0])], n)
