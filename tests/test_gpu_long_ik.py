"""GPU parity of the batched local IK on chains with more than ten input joints (rdyn_long_ik.hip): computeLocalIk /
computeWeigthedLocalIk (primitives_impl.h:1398-1468) with the Levenberg term of rdyn_local_ik_damped.  Such chains have no reduced
companion.  The reference's default build has no bound on the number of joints (rosdyn_core/CMakeLists.txt:12-16).

References: scipy's BVLS on the damped, weighted least-squares form of one QP update; the C oracle's loop where it reaches (at most 16
input joints); a numpy restatement of the whole loop (BVLS per update, the oracle's FK and Jacobian) beyond that."""
import numpy as np
import pytest

from rosdyn_amd.urdf_gen import generated_long_chain, generated_revolute_chain

pytestmark = pytest.mark.gpu
WEIGHT = (1.0, 2.0, 0.5, 0.3, 1.5, 0.8)


def _case(name):
    from oracle.oracle import OracleChain
    from rosdyn_amd import Chain
    inputs = None
    if name.startswith("rev"):
        nj = int(name[3:])
        xml, base, tool = generated_revolute_chain(nj, 1000 + nj), "l0", "l%d" % nj
    elif name == "gen20_all":
        xml, base, tool = generated_long_chain(20, 2020), "l0", "l20"
    elif name == "gen32_all":
        xml, base, tool = generated_long_chain(32, 3232), "l0", "l32"
    else:  # "gen20_permuted": 12 of the 14 moving joints, out of chain order
        xml, base, tool = generated_long_chain(20, 2020), "l0", "l20"
        inputs = ["j13", "j0", "j9", "j4", "j16", "j1", "j7", "j19", "j3", "j10", "j6", "j12"]
    chain, ref = Chain(xml, base, tool), OracleChain(xml, base, tool, input_joint_names=inputs)
    if inputs:
        assert chain.setInputJointsName(inputs)
    assert chain.getJointsNumber() > 10 and chain.getActiveJointsNumber() == ref.n > 10
    return chain, ref


def _poses(ref, N, spread, seed):
    """Reachable goals well inside the limits, seeds displaced by ~spread rad."""
    from rosdyn_amd.samples import uniform_pm1
    lo, hi = np.array(ref.spec.q_min), np.array(ref.spec.q_max)
    q_goal = np.clip(uniform_pm1(seed, (N, ref.n)), lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo))
    seeds = np.clip(q_goal + spread * uniform_pm1(seed + 1, (N, ref.n)), lo, hi)
    return q_goal, seeds, ref.fk(q_goal)[:, -1], lo, hi


def _run(torch, chain, T, seeds, layout="sample", **kw):
    Tt = np.ascontiguousarray(T.transpose(0, 2, 1))   # (N, 4, 3): the getTransformation record
    if layout == "element":
        tT = torch.from_numpy(np.ascontiguousarray(np.moveaxis(Tt, 0, -1))).cuda()
        ts = torch.from_numpy(np.ascontiguousarray(seeds.T)).cuda()
    else:
        tT, ts = torch.from_numpy(Tt).cuda(), torch.from_numpy(np.ascontiguousarray(seeds)).cuda()
    sol, st, it = chain.computeLocalIk(tT, ts, layout=layout, **kw)
    sol = sol.cpu().numpy()
    return (sol.T if layout == "element" else sol), st.cpu().numpy(), it.cpu().numpy()


def _bvls_step(J, e, w, lam, lo, hi):
    """argmin 1/2 dq'(J'WJ + lam^2 I)dq - (J'We)'dq  s.t. lo <= dq <= hi, as [sqrt(W) J; lam I] dq ~ [sqrt(W) e; 0]."""
    from scipy.optimize import lsq_linear
    sw = np.sqrt(np.asarray(w, dtype=np.float64))
    n = J.shape[1]
    A = np.vstack([sw[:, None] * J, lam * np.eye(n)])
    rhs = np.concatenate([sw * e, np.zeros(n)])
    return lsq_linear(A, rhs, bounds=(lo, hi), method="bvls", tol=1e-12).x


def _loop_ref(ref, T, seeds, w, toll, lam, max_iter, lo, hi):
    """The whole loop of rdyn.h restated: the oracle's FK, getFrameDistance and Jacobian, one BVLS per update."""
    from oracle.oracle import frame_distance
    N = len(seeds)
    sol, st, its = seeds.copy(), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for s in range(N):
        q = seeds[s].copy()
        it = 0
        while True:
            e = frame_distance(T[s], ref.fk(q[None])[0, -1])
            if np.linalg.norm(np.asarray(w) * e) < toll:
                st[s] = 1
                break
            if it >= max_iter:
                break
            J = ref.jacobian(q[None])[0]
            q = q + _bvls_step(J, e, w, lam, lo - q, hi - q)
            it += 1
        sol[s], its[s] = q, it
    return sol, st, its


CASES = ["rev14", "rev20", "rev32", "gen32_all", "gen20_permuted"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("lam", [1e-3, 0.1])
def test_one_update_is_the_exact_qp_minimiser(case, lam):
    torch = pytest.importorskip("torch")
    from oracle.oracle import frame_distance
    chain, ref = _case(case)
    N, n = 130, ref.n
    q_goal, seeds, T, lo, hi = _poses(ref, N, 0.3, 31)
    # some seeds on a bound, some outside one (the QP then starts from the clamped step)
    rng = np.random.default_rng(5)
    for s in range(N):
        ks = rng.choice(n, size=3, replace=False)
        seeds[s, ks[0]] = lo[ks[0]] if s % 2 else hi[ks[0]]
        if s % 3 == 0:
            seeds[s, ks[1]] = hi[ks[1]] + 0.02
        if s % 5 == 0:
            seeds[s, ks[2]] = lo[ks[2]] - 0.01
    sol, st, it = _run(torch, chain, T, seeds, toll=1e-14, max_iterations=1, damping=lam, weight=WEIGHT)
    assert (it == 1).all() and (st == 0).all(), (np.unique(st), np.unique(it))
    J = ref.jacobian(seeds)
    Tb = ref.fk(seeds)[:, -1]
    n_active = 0
    for s in range(N):
        e = frame_distance(T[s], Tb[s])
        dq_ref = _bvls_step(J[s], e, WEIGHT, lam, lo - seeds[s], hi - seeds[s])
        dq = sol[s] - seeds[s]
        assert np.linalg.norm(dq - dq_ref) <= 1e-9 * max(1.0, np.linalg.norm(dq_ref)), (s, np.linalg.norm(dq - dq_ref))
        n_active += int(np.any(np.isclose(dq_ref, lo - seeds[s], atol=1e-12) | np.isclose(dq_ref, hi - seeds[s], atol=1e-12)))
    assert (sol >= lo - 1e-12).all() and (sol <= hi + 1e-12).all()
    assert n_active > N // 4, n_active   # the bounds really took part


@pytest.mark.parametrize("case", ["rev14", "gen20_all"])
@pytest.mark.parametrize("layout", ["sample", "element"])
def test_matches_the_oracle_loop(case, layout):
    """14 input joints: within the oracle's reach (IK_MAX_N = 16)."""
    torch = pytest.importorskip("torch")
    chain, ref = _case(case)
    assert ref.n == 14
    N = 1000                         # a ragged last wave
    q_goal, seeds, T, lo, hi = _poses(ref, N, 0.1, 41)
    kw = dict(toll=1e-6, max_iterations=30, damping=1e-3, weight=WEIGHT)
    sol, st, it = _run(torch, chain, T, seeds, layout, **kw)
    rsol, rst, rit = ref.local_ik(T, seeds, weight=np.array(WEIGHT), toll=1e-6, max_iter=30, damping=1e-3)
    conv = (rst == 1) & (rit <= 8)
    assert conv.mean() > 0.8, conv.mean()
    assert (st[conv] == 1).all()
    assert np.array_equal(it[conv], rit[conv])
    assert np.abs(sol[conv] - rsol[conv]).max() < 1e-9
    assert (st != rst).mean() < 0.05, (st != rst).mean()
    assert (sol >= lo - 1e-12).all() and (sol <= hi + 1e-12).all()


@pytest.mark.parametrize("case", ["rev20", "rev32", "gen32_all", "gen20_permuted"])
def test_matches_the_restated_loop_beyond_the_oracle(case):
    torch = pytest.importorskip("torch")
    from oracle.oracle import frame_distance
    chain, ref = _case(case)
    N, toll, lam = 200, 1e-6, 1e-3
    q_goal, seeds, T, lo, hi = _poses(ref, N, 0.1, 51)
    sol, st, it = _run(torch, chain, T, seeds, toll=toll, max_iterations=20, damping=lam, weight=WEIGHT)
    rsol, rst, rit = _loop_ref(ref, T, seeds, WEIGHT, toll, lam, 20, lo, hi)
    conv = (rst == 1) & (rit <= 8)
    assert conv.mean() > 0.8, conv.mean()
    assert (st[conv] == 1).all()
    assert np.array_equal(it[conv], rit[conv])
    assert np.abs(sol[conv] - rsol[conv]).max() < 1e-9
    assert (st != rst).mean() < 0.05, (st != rst).mean()
    assert (sol >= lo - 1e-12).all() and (sol <= hi + 1e-12).all()
    # every converged pose is a solution, measured through the product's getTransformation
    ok = st == 1
    Tp = chain.getTransformation(torch.from_numpy(np.ascontiguousarray(sol[ok])).cuda()).cpu().numpy().transpose(0, 2, 1)
    werr = [np.linalg.norm(np.asarray(WEIGHT) * frame_distance(a, b)) for a, b in zip(T[ok], Tp)]
    assert max(werr) < toll


@pytest.mark.parametrize("case", ["rev20", "gen32_all"])
def test_status_contract_aliasing_and_graph_replay(case):
    torch = pytest.importorskip("torch")
    chain, ref = _case(case)
    N = 300
    q_goal, seeds, T, lo, hi = _poses(ref, N, 0.1, 61)
    at_goal = np.arange(N) % 3 == 0
    seeds[at_goal] = q_goal[at_goal]
    Tt = torch.from_numpy(np.ascontiguousarray(T.transpose(0, 2, 1))).cuda()
    # undamped: J'WJ is singular (more than six input joints) -- a pose solved at its seed is status 1 after 0 updates, any other -1
    ts = torch.from_numpy(np.ascontiguousarray(seeds)).cuda()
    sol, st, it = chain.computeLocalIk(Tt, ts, toll=1e-8, max_iterations=20, damping=0.0, out=ts)   # sol aliases the seeds
    st, it = st.cpu().numpy(), it.cpu().numpy()
    assert (st[at_goal] == 1).all() and (it[at_goal] == 0).all()
    assert (st[~at_goal] == -1).all() and (it[~at_goal] == 0).all()
    assert np.array_equal(sol.cpu().numpy(), seeds)
    # damped, aliased: bit-identical to separate buffers
    kw = dict(toll=1e-8, max_iterations=20, damping=1e-3)
    ts = torch.from_numpy(np.ascontiguousarray(seeds)).cuda()
    sol_a, st_a, it_a = chain.computeLocalIk(Tt, ts, **kw)
    sol_b, st_b, it_b = chain.computeLocalIk(Tt, ts.clone(), out=ts.clone(), **kw)
    assert (st_a.cpu().numpy()[~at_goal] == 1).mean() > 0.9
    al = ts.clone()
    sol_c, st_c, it_c = chain.computeLocalIk(Tt, al, out=al, **kw)
    assert torch.equal(sol_a, sol_c) and torch.equal(st_a, st_c) and torch.equal(it_a, it_c)
    assert torch.equal(sol_a, sol_b) and torch.equal(st_a, st_b)
    # a single-stream graph capture and replay: bit-identical to the eager call
    seeds_g = ts.clone()
    sol_g = torch.empty_like(ts)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    holder = {}
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            holder["ik"] = chain.computeLocalIk(Tt, seeds_g, out=sol_g, **kw)
    seeds_g.copy_(ts)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(sol_g, sol_a) and torch.equal(holder["ik"][1], st_a) and torch.equal(holder["ik"][2], it_a)


NARROW = (3, 7, 11)   # joints of the 14-revolute chain given the range [0.01, 0.05]


@pytest.mark.parametrize("lam", [1e-3, 0.1])
def test_one_update_with_narrow_ranges_and_seeds_outside_them(lam):
    """Seeds below or above a joint range narrower than the step: the QP starts that joint at the near bound, releases it, and
    the solve then carries it to the far bound.  The update must still be the exact minimiser."""
    import re
    torch = pytest.importorskip("torch")
    from oracle.oracle import OracleChain, frame_distance
    from rosdyn_amd import Chain
    xml = generated_revolute_chain(14, 1014)
    for k in NARROW:
        xml = re.sub(r"(<joint name='j%d' .*?<limit lower=')-3(' upper=')3(')" % k, r"\g<1>0.01\g<2>0.05\g<3>", xml, count=1)
    chain, ref = Chain(xml, "l0", "l14"), OracleChain(xml, "l0", "l14")
    N = 400
    q_goal, seeds, T, lo, hi = _poses(ref, N, 0.3, 71)
    assert all(lo[k] == 0.01 and hi[k] == 0.05 for k in NARROW)
    rng = np.random.default_rng(9)
    for k in NARROW:
        side = rng.integers(0, 3, N)
        seeds[:, k] = np.where(side == 0, lo[k] - rng.uniform(0, 0.15, N), np.where(side == 1, hi[k] + rng.uniform(0, 0.15, N), seeds[:, k]))
    sol, st, it = _run(torch, chain, T, seeds, toll=1e-14, max_iterations=1, damping=lam, weight=WEIGHT)
    assert (it == 1).all() and (st == 0).all(), (np.unique(st), np.unique(it))
    J = ref.jacobian(seeds)
    Tb = ref.fk(seeds)[:, -1]
    crossed = 0
    for s in range(N):
        dq_ref = _bvls_step(J[s], frame_distance(T[s], Tb[s]), WEIGHT, lam, lo - seeds[s], hi - seeds[s])
        dq = sol[s] - seeds[s]
        assert np.linalg.norm(dq - dq_ref) <= 1e-9 * max(1.0, np.linalg.norm(dq_ref)), (s, np.linalg.norm(dq - dq_ref))
        for k in NARROW:
            crossed += int((seeds[s, k] < lo[k] and abs(dq_ref[k] - (hi[k] - seeds[s, k])) < 1e-12)
                           or (seeds[s, k] > hi[k] and abs(dq_ref[k] - (lo[k] - seeds[s, k])) < 1e-12))
    assert crossed > N // 10, crossed   # the far bound really was reached from outside the range
    assert (sol >= lo - 1e-12).all() and (sol <= hi + 1e-12).all()


def test_fixed_joints_among_the_inputs():
    """setInputJointsName accepts fixed joints: 10 fixed + 5 moving input joints take the long route with 5 QP variables.  Undamped,
    the 6 x 6 system of 5 free joints is singular: status -1 (not a step); damped, the loop converges."""
    torch = pytest.importorskip("torch")
    from oracle.oracle import frame_distance
    from rosdyn_amd import Chain
    from rosdyn_amd.samples import uniform_pm1
    chain = Chain(generated_long_chain(32, 3232), "l0", "l32")
    fixed = ["j%d" % i for i in range(32) if i % 3 == 2]
    moving = ["j0", "j1", "j3", "j4", "j6"]
    assert chain.setInputJointsName(fixed + moving)
    n, N = 15, 256
    q_goal = np.zeros((N, n))
    q_goal[:, 10:] = uniform_pm1(81, (N, 5))
    seeds = q_goal.copy()
    seeds[:, 10:] += 0.1 * uniform_pm1(82, (N, 5))
    at_goal = np.arange(N) % 4 == 0
    seeds[at_goal] = q_goal[at_goal]
    T = chain.getTransformation(torch.from_numpy(q_goal).cuda())
    ts = torch.from_numpy(np.ascontiguousarray(seeds)).cuda()
    sol, st, it = chain.computeLocalIk(T, ts, toll=1e-8, max_iterations=50, damping=0.0)
    st, it = st.cpu().numpy(), it.cpu().numpy()
    assert (st[at_goal] == 1).all() and (st[~at_goal] == -1).all() and (it == 0).all()
    assert np.array_equal(sol.cpu().numpy(), seeds)
    sol, st, it = chain.computeLocalIk(T, ts, toll=1e-8, max_iterations=100, damping=1e-2)
    sol, st = sol.cpu().numpy(), st.cpu().numpy()
    assert (st == 1).mean() > 0.9, np.unique(st, return_counts=True)
    assert np.array_equal(sol[:, :10], seeds[:, :10])          # fixed joints are no QP variables
    ok = st == 1
    Tp = chain.getTransformation(torch.from_numpy(np.ascontiguousarray(sol[ok])).cuda()).cpu().numpy().transpose(0, 2, 1)
    Tg = T.cpu().numpy().transpose(0, 2, 1)[ok]
    assert max(np.linalg.norm(frame_distance(a, b)) for a, b in zip(Tg, Tp)) < 1e-8
