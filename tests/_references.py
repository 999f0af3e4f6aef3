"""Test support: host references and bounds -- the oracle's forward dynamics, the integrators and their transposes in numpy, the exact
derivative reference with its cache, and the library-side closures the numpy adjoints are composed from."""
import numpy as np

from _arrays import DT, EPS, REVOLUTE, _dev, _dev_w, _inf, _mat, _rollout, _rollout_inputs


def _solver_bound_check(ddq, M, h, tau, what):
    ddq_host = np.linalg.solve(M, (tau - h)[:, :, None])[:, :, 0]
    cond = np.linalg.cond(M)
    ratio = _inf(ddq - ddq_host) / (EPS * cond * np.maximum(1.0, _inf(ddq_host)))
    print("%s: solver ratio max %.3g (bound 64), cond2 %.3g .. %.3g" % (what, ratio.max(), cond.min(), cond.max()))
    assert (ratio <= 64.0).all(), (what, float(ratio.max()), int(np.argmax(ratio)))


def _input_types(chain):
    """rdyn_joint_type of every input joint, in input order"""
    from rosdyn_amd._lib import lib
    L, h = lib(), chain._h
    kind = {L.rdyn_chain_joint_name(h, j).decode(): L.rdyn_chain_joint_type(h, j) for j in range(L.rdyn_chain_joints_number(h))}
    return [kind[name] for name in chain.getActiveJointsName()]


def _spectral(ref, q, dq, ddq, k, points):
    """d tau / d q_k of every sample by spectral differentiation over `points` equispaced samples of q_k: (N, n)"""
    N, n = q.shape
    Q = np.repeat(q[None], points, axis=0)
    Q[:, :, k] += (2.0 * np.pi / points) * np.arange(points)[:, None]
    T = ref.joint_torque(Q.reshape(-1, n), np.tile(dq, (points, 1)), np.tile(ddq, (points, 1))).reshape(points, N, n)
    c = np.fft.fft(T, axis=0) / points
    freq = np.fft.fftfreq(points, 1.0 / points)
    c[points // 2] = 0.0   # the Nyquist mode has no derivative on the grid (and no content: degree <= 2)
    return (1j * freq[:, None, None] * c).sum(axis=0).real   # the grid starts AT q_k: the derivative there is sum_m i m c_m


def _central(ref, q, dq, ddq, k, which):
    e = np.zeros_like(q)
    e[:, k] = 1.0
    if which == 0:
        return 0.5 * (ref.joint_torque(q + e, dq, ddq) - ref.joint_torque(q - e, dq, ddq))
    return 0.5 * (ref.joint_torque(q, dq + e, ddq) - ref.joint_torque(q, dq - e, ddq))


def _reference(ref, types, q, dq, ddq):
    """(Dq_ref, Dv_ref, tau_ref, construction gap): D[s, i, k] = d tau_i / d x_k"""
    N, n = q.shape
    Dq, Dv = np.zeros((N, n, n)), np.zeros((N, n, n))
    gap = np.zeros(N)
    for k in range(n):
        if types[k] == REVOLUTE:
            Dq[:, :, k] = _spectral(ref, q, dq, ddq, k, 8)
            gap = np.maximum(gap, _inf(Dq[:, :, k] - _spectral(ref, q, dq, ddq, k, 16)))
        else:
            Dq[:, :, k] = _central(ref, q, dq, ddq, k, 0)
        Dv[:, :, k] = _central(ref, q, dq, ddq, k, 1)
    return Dq, Dv, ref.joint_torque(q, dq, ddq), gap


def _oracle_fd(ref, perturb=None):
    def fd(q, dq, tau):
        M = ref.joint_inertia(q)
        h = ref.joint_torque(q, dq, np.zeros_like(q))
        a = np.linalg.solve(M, (tau - h)[:, :, None])[:, :, 0]
        if perturb is not None:
            a = a * (1.0 + 1e-11 * perturb.uniform(-1.0, 1.0, a.shape))
        return a
    return fd


def _np_step(fd, q, dq, tau, dt, integrator):
    if integrator == "semi_implicit_euler":
        dq1 = dq + dt * fd(q, dq, tau)
        return q + dt * dq1, dq1
    a1 = fd(q, dq, tau)
    v2 = dq + 0.5 * dt * a1
    a2 = fd(q + 0.5 * dt * dq, v2, tau)
    v3 = dq + 0.5 * dt * a2
    a3 = fd(q + 0.5 * dt * v2, v3, tau)
    v4 = dq + dt * a3
    a4 = fd(q + dt * v3, v4, tau)
    return q + dt * (dq / 6 + v2 / 3 + v3 / 3 + v4 / 6), dq + dt * (a1 / 6 + a2 / 3 + a3 / 3 + a4 / 6)


def _np_rollout(fd, q, dq, tau, dt, T, integrator):
    """tau: (T, N, n), or (N, n) held for all steps"""
    for t in range(T):
        q, dq = _np_step(fd, q, dq, tau[t] if tau.ndim == 3 else tau, dt, integrator)
    return q, dq


def _euler_residual_check(torch, chain, ref, name, N, layout, seed, inputs=None):
    """inputs: None (this module's inputs for the chain `name`), or (q0, dq0, tau) with tau of shape (1, N, n) and `name` a label"""
    q0, dq0, tau = inputs if inputs is not None else _rollout_inputs(name, ref.n, N, 1, seed=seed)
    q1, dq1, st = _rollout(torch, chain, q0, dq0, tau, DT, "semi_implicit_euler", layout)
    assert (st == 1).all(), np.unique(st)
    ddq = (dq1 - dq0) / DT
    M = ref.joint_inertia(q0)
    h = ref.joint_torque(q0, dq0, np.zeros_like(q0))
    Minf = np.abs(M).sum(axis=2).max(axis=1)
    res = _inf(np.einsum("sij,sj->si", M, ddq) + h - tau[0])
    bound = 1e-11 * (Minf * _inf(ddq) + _inf(tau[0]) + _inf(h)) + (4 * EPS / DT) * (_inf(dq0) + DT * _inf(ddq)) * Minf
    print("%s %s N=%d: residual/bound max %.3g" % (name, layout, N, (res / bound).max()))
    assert (res <= bound).all(), (float((res / bound).max()), int(np.argmax(res / bound)))
    assert (_inf(q1 - (q0 + DT * dq1)) <= 4 * EPS * (_inf(q0) + DT * _inf(dq1))).all()


def _oracle_fd_c(ref, specs, perturb=None):
    from oracle.oracle import components_regressor
    fd = _oracle_fd(ref, perturb)
    return lambda q, dq, tau: fd(q, dq, tau - components_regressor(specs, ref.n, q, dq)[1])


def _norm_inf(M):
    return np.abs(M).sum(axis=2).max(axis=1)


def _derivative_residual_ratios(ref, types, q, dq, ddq, Xq, Xv, Minv, slopes=None, cached=None):
    """worst ratio residual / scale per output over the samples given, and the construction gap of the reference.
    cached: None, or what test_gpu_forward_dynamics_vjp._cached_reference returns for these very (q, dq, ddq) -- (M_ref, Dq_ref, Dv_ref,
    tau_ref, gscale), its construction gap asserted there -- so that the reference is computed once for both modules' residuals."""
    N, n = q.shape
    if cached is None:
        Dq_ref, Dv_ref, tau_ref, gap = _reference(ref, types, q, dq, ddq)
        gscale = np.maximum(_inf(Dq_ref), _inf(Dv_ref)) + _inf(tau_ref)
        assert (gap <= 1e-12 * gscale).all(), ("spectral reference, 8 against 16 points", float((gap / gscale).max()))
        M = ref.joint_inertia(q)
    else:
        M, Dq_ref, Dv_ref, tau_ref = cached[:4]
        Dq_ref, Dv_ref = Dq_ref.copy(), Dv_ref.copy()
    if slopes is not None:
        idx = np.arange(n)
        Dq_ref[:, idx, idx] += slopes[0]
        Dv_ref[:, idx, idx] += slopes[1]
    mn = _norm_inf(M)
    out = {}
    for what, X, D in (("dddq_dq", Xq, Dq_ref), ("dddq_dv", Xv, Dv_ref)):
        res = _inf(np.einsum("sij,sjk->sik", M, X) + D)
        out[what] = float((res / (mn * _inf(X) + _inf(D) + _inf(tau_ref))).max())
    res = _inf(np.einsum("sij,sjk->sik", M, Minv) - np.eye(n)[None])
    out["minv"] = float((res / (mn * _inf(Minv) + 1.0)).max())
    return out


_REF = {}


def _cached_reference(key, ref, types, q, dq, ddq):
    """the oracle's M, D and tau at the library's ddq: computed once per (chain, inputs) and shared by the layouts (the same ddq bits)"""
    if key not in _REF:
        Dq_ref, Dv_ref, tau_ref, gap = _reference(ref, types, q, dq, ddq)
        gscale = np.maximum(_inf(Dq_ref), _inf(Dv_ref)) + _inf(tau_ref)
        assert (gap <= 1e-12 * gscale).all(), ("spectral reference, 8 against 16 points", float((gap / gscale).max()))
        for x in (Dq_ref, Dv_ref, tau_ref, gscale):
            x.setflags(write=False)
        M = ref.joint_inertia(q)
        M.setflags(write=False)
        _REF[key] = (ddq.copy(), M, Dq_ref, Dv_ref, tau_ref, gscale)
    assert np.array_equal(_REF[key][0], ddq), "the layouts must give the same ddq bits"
    return _REF[key][1:]


def _vjp_residual_ratios(cached, a, qb, vb, tb, slopes=None):
    M, Dq_ref, Dv_ref, tau_ref, gscale = cached
    n = a.shape[1]
    if slopes is not None:
        idx = np.arange(n)
        Dq_ref, Dv_ref = Dq_ref.copy(), Dv_ref.copy()
        Dq_ref[:, idx, idx] += slopes[0]
        Dv_ref[:, idx, idx] += slopes[1]
    mn = np.abs(M).sum(axis=2).max(axis=1)
    out = {"tau_bar": float((_inf(np.einsum("sij,sj->si", M, tb) - a) / (mn * _inf(tb) + _inf(a))).max())}
    l1 = np.abs(tb).sum(axis=1)
    l1 = np.where(l1 > 0, l1, 1.0)
    out["q_bar"] = float((_inf(qb + np.einsum("sik,si->sk", Dq_ref, tb)) / (gscale * l1)).max())
    out["dq_bar"] = float((_inf(vb + np.einsum("sik,si->sk", Dv_ref, tb)) / (gscale * l1)).max())
    return out


B4 = (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0)


def _np_stage_states(fd, q, v, tau, dt):
    X = [(q, v)]
    for c in (0.5 * dt, 0.5 * dt, dt):
        a = fd(X[-1][0], X[-1][1], tau)
        X.append((q + c * X[-1][1], v + c * a))
    return X


def _np_step_adjoint(vjp, fd, q, v, tau, lq, lv, dt, integrator):
    """(lq, lv, gtau) of one backward step, by the formulas of include/rdyn.h in their order"""
    if integrator == "semi_implicit_euler":
        lvs = lv + dt * lq
        qb, vb, tb = vjp(q, v, tau, dt * lvs)
        return lq + qb, lvs + vb, tb
    X = _np_stage_states(fd, q, v, tau, dt)
    kq = [dt * b * lq for b in B4]
    kv = [dt * b * lv for b in B4]
    xq, xv, gtau = lq.copy(), lv.copy(), np.zeros_like(lq)
    c = (None, 0.5 * dt, 0.5 * dt, dt)
    for i in (3, 2, 1, 0):
        qb, vb, tb = vjp(X[i][0], X[i][1], tau, kv[i])
        Xq, Xv = qb, kq[i] + vb
        gtau = gtau + tb
        xq, xv = xq + Xq, xv + Xv
        if i > 0:
            kq[i - 1] = kq[i - 1] + c[i] * Xq
            kv[i - 1] = kv[i - 1] + c[i] * Xv
    return xq, xv, gtau


def _np_adjoint(vjp, fd, q0, dq0, tau, q_traj, dq_traj, gq_end, gdq_end, dt, integrator, gq_traj=None, gdq_traj=None):
    """(gq0, gdq0, gtau (T, N, n)) over the whole horizon; x_t from the trajectory given (record k = x_{k + 1})"""
    T = tau.shape[0]
    lq, lv = gq_end.copy(), gdq_end.copy()
    if gq_traj is not None and T > 0:
        lq, lv = lq + gq_traj[T - 1], lv + gdq_traj[T - 1]
    gtau = np.zeros_like(tau)
    for t in range(T - 1, -1, -1):
        q, v = (q0, dq0) if t == 0 else (q_traj[t - 1], dq_traj[t - 1])
        lq, lv, gtau[t] = _np_step_adjoint(vjp, fd, q, v, tau[t], lq, lv, dt, integrator)
        if t >= 1 and gq_traj is not None:
            lq, lv = lq + gq_traj[t - 1], lv + gdq_traj[t - 1]
    return lq, lv, gtau


def _lib_fd(torch, chain, components=None):
    def fd(q, v, tau):
        a, st = chain.getJointAcceleration(_dev(torch, q, "sample"), _dev(torch, v, "sample"), _dev(torch, tau, "sample"), components=components)
        assert (st.cpu().numpy() == 1).all()
        return a.cpu().numpy()
    return fd


def _lib_vjp(torch, chain, components=None):
    def vjp(q, v, tau, seed):
        out = chain.getJointAccelerationVjp(*(_dev(torch, x, "sample") for x in (q, v, tau, seed)), components=components)
        assert (out[0].cpu().numpy() == 1).all()
        return tuple(t.cpu().numpy() for t in out[1:])
    return vjp


def _lib_abs_vjp(torch, chain, components=None):
    """the product on magnitudes: |dddq_dq|' m, |dddq_dv|' m, |minv| m -- the sum of the absolute terms of every entry of the product"""
    def vjp(q, v, tau, m):
        out = chain.getJointAccelerationDerivatives(*(_dev(torch, x, "sample") for x in (q, v, tau)), components=components)
        Xq, Xv, Mi = (np.abs(_mat(t, "sample")) for t in out[2:])   # [s, i, k]
        return np.einsum("sik,si->sk", Xq, m), np.einsum("sik,si->sk", Xv, m), np.einsum("sik,si->sk", Mi, m)
    return vjp


def _tau_e(torch, chain0, q, W):
    """the library's own wrench torque at host arrays: getJointTorqueExt(q, 0, 0, W) on the zero-gravity chain"""
    tq = _dev(torch, q, "sample")
    z = torch.zeros_like(tq)
    return chain0.getJointTorqueExt(tq, z, z, _dev_w(torch, W, "sample")).cpu().numpy()


def _bound(torch, chain, q, dq, tau, tau_e, ddq):
    """64 eps (cond2(M) max(1, |ddq|_inf) + |M^-1|_2 (|tau|_2 + |h|_2 + |tau_E|_2)) per sample, M and h the library's own"""
    tq, tdq = _dev(torch, q, "sample"), _dev(torch, dq, "sample")
    M = chain.getJointInertia(tq).cpu().numpy()
    h = chain.getJointTorqueNonLinearPart(tq, tdq).cpu().numpy()
    sv = np.linalg.svd(M, compute_uv=False)
    l2 = lambda x: np.sqrt((x * x).sum(axis=1))
    return 64.0 * EPS * (sv[:, 0] / sv[:, -1] * np.maximum(1.0, _inf(ddq)) + (l2(tau) + l2(h) + l2(tau_e)) / sv[:, -1])


class _WrenchTorque:
    """the oracle's wrench torque tau_E(q) of fixed wrenches W in the shape of an oracle chain, for _reference"""

    def __init__(self, ref, W):
        self.ref, self.W = ref, W

    def joint_torque(self, q, dq, ddq):
        Wt = np.tile(self.W, (len(q) // len(self.W), 1, 1))
        z = np.zeros_like(q)
        return self.ref.joint_torque(q, z, z, ext=Wt) - self.ref.joint_torque(q, z, z)


def _wrench_matrix(torch, chain0, q, L):
    """A[s, i, 6 l + e] = tau_E,i of the unit wrench e on link l: the library's own getJointTorqueExt on the zero-gravity chain"""
    N, n = q.shape
    tq = _dev(torch, q, "sample")
    z = torch.zeros_like(tq)
    A = np.zeros((N, n, 6 * L))
    for col in range(6 * L):
        U = torch.zeros((N, L, 6), dtype=torch.float64, device="cuda")
        U[:, col // 6, col % 6] = 1.0
        A[:, :, col] = chain0.getJointTorqueExt(tq, z, z, U).cpu().numpy()
    return A


def _oracle_fd_ext(ref, W):
    def fd(q, dq, tau):
        M = ref.joint_inertia(q)
        h = ref.joint_torque(q, dq, np.zeros_like(q), ext=W)
        return np.linalg.solve(M, (tau - h)[:, :, None])[:, :, 0]
    return fd


# chain: worst err(H) / scale on the oracle (semi-implicit Euler, RK4): the table in the docstring of test_parameter_gradient_inputs.py
ORACLE_WORST = {
    "planar_2r": (7.839e-05, 8.097e-05), "ur10_like": (5.840e-05, 6.196e-05), "panda_like": (4.089e-04, 3.272e-04),
}
