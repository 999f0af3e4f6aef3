"""GPU tests of the normal equations wider than 111 columns: the column-panel Gram (rdyn_panel_gram.hip) behind rdyn_gram_wide,
rdyn_regressor_gram_wide and rdyn_identification_gram_wide, against numpy and the C oracle.  The identification step the regressor
exists for stacks getRegressor rows of whatever chain it is given (the reference's default build has no bound on the number of
joints, rosdyn_core/CMakeLists.txt:12-16)."""
import os

import numpy as np
import pytest

from conftest import FIXTURES
from _chains import WIDE_GRAV as GRAV, _chain_case, _ur6
from rosdyn_amd.urdf_gen import generated_revolute_chain

pytestmark = pytest.mark.gpu


def _fro(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _full(G, c, bb):
    """[G c; c' bb] on the host."""
    G = G.cpu().numpy()
    P = G.shape[0]
    out = np.zeros((P + 1, P + 1))
    out[:P, :P], out[:P, P], out[P, :P], out[P, P] = G, c.cpu().numpy(), c.cpu().numpy(), float(bb.cpu()[0])
    return out


def _gram_wide_raw(torch, A, rows, lda, n_cols, b, out, accumulate):
    from rosdyn_amd._lib import check, lib
    G, c, bb = out
    ws = torch.empty((lib().rdyn_gram_wide_workspace_bytes(n_cols),), dtype=torch.uint8, device="cuda")
    check(lib().rdyn_gram_wide(A.data_ptr(), rows, lda, n_cols, b.data_ptr() if b is not None else None, G.data_ptr(), c.data_ptr(),
                               bb.data_ptr(), 1 if accumulate else 0, ws.data_ptr(), ws.numel(), -1,
                               torch.cuda.current_stream().cuda_stream))
    return G, c, bb


@pytest.mark.parametrize("n_cols", [1, 17, 111, 112, 200, 321, 415])
@pytest.mark.parametrize("with_b", [True, False])
def test_gram_wide_matches_numpy(n_cols, with_b):
    """rdyn_gram_wide on seeded random matrices: ragged row counts, lda > rows, accumulate; bitwise reproducible."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.gram import gram_wide
    rng = np.random.default_rng(1000 + n_cols)
    for rows, lda in ((3001, 3001), (1237, 1250)):
        Ah = rng.normal(size=(n_cols, lda))              # column-major rows x n_cols with leading dimension lda
        bh = rng.normal(size=rows) if with_b else None
        A = torch.from_numpy(Ah).cuda()
        b = torch.from_numpy(bh).cuda() if with_b else None
        out = tuple(torch.full(s, np.nan, dtype=torch.float64, device="cuda") for s in ((n_cols, n_cols), (n_cols,), (1,)))
        G, c, bb = _gram_wide_raw(torch, A, rows, lda, n_cols, b, out, False)
        M = Ah[:, :rows].T
        Gr = M.T @ M
        assert _fro(G.cpu().numpy(), Gr) <= 1e-12
        if with_b:
            assert _fro(c.cpu().numpy(), M.T @ bh) <= 1e-12 and abs(float(bb.cpu()[0]) - bh @ bh) <= 1e-12 * (bh @ bh)
        else:
            assert not c.abs().max().item() and not bb.abs().max().item()
        first = [t.clone() for t in (G, c, bb)]
        _gram_wide_raw(torch, A, rows, lda, n_cols, b, out, False)
        assert all(torch.equal(x, y) for x, y in zip(first, (G, c, bb)))
        _gram_wide_raw(torch, A, rows, lda, n_cols, b, out, True)       # accumulate: twice the Gram
        assert _fro(G.cpu().numpy(), 2 * Gr) <= 1e-12
        if rows == lda:
            G2, c2, bb2 = gram_wide(A.view(n_cols, rows), b)            # the Python binding (contiguous, lda = rows)
            assert torch.equal(G2, first[0]) and torch.equal(c2, first[1]) and torch.equal(bb2, first[2])
    if n_cols == 111:
        from rosdyn_amd.gram import gram
        A = torch.from_numpy(np.ascontiguousarray(Ah[:, :rows])).cuda()
        Gn, cn, _ = gram(A, b)
        Gw, cw, _ = gram_wide(A, b)
        assert _fro(Gw.cpu().numpy(), Gn.cpu().numpy()) <= 1e-13
        if with_b:
            assert _fro(cw.cpu().numpy(), cn.cpu().numpy()) <= 1e-13


@pytest.mark.parametrize("case", ["rev12", "rev14", "rev20", "rev32", "gen20_twelve_permuted"])
def test_regressor_gram_wide_matches_oracle(case):
    """A = regressor(q, dq, ddq).reshape(N n, P): A'A, A'tau, tau'tau for chains of 12 to 32 input joints, both input layouts, the
    default chunk and a small one with a ragged last chunk, accumulation, N = 0."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.samples import trajectory_batch
    chain, ref = _chain_case(case)
    n, P, N = ref.n, ref.P, 250
    assert n > 11 and chain.getActiveJointsNumber() == n
    q, dq, ddq = trajectory_batch(81, N, n)
    tau = ref.joint_torque(q, dq, ddq) + 1e-3 * np.random.default_rng(3).normal(size=(N, n))
    A = ref.regressor(q, dq, ddq).reshape(N * n, P)
    M = np.column_stack([A, tau.reshape(-1)])
    Fr = M.T @ M
    ts = [torch.from_numpy(x).cuda() for x in (q, dq, ddq, tau)]
    te = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in (q, dq, ddq, tau)]
    for args, layout in ((ts, "sample"), (te, "element")):
        for chunk in (0, 96):
            G, c, bb = chain.getRegressorGramWide(*args, layout=layout, chunk_samples=chunk)
            F = _full(G, c, bb)
            assert _fro(F[:P, :P], Fr[:P, :P]) <= 1e-10 and _fro(F[:P, P], Fr[:P, P]) <= 1e-10, (layout, chunk)
            assert abs(F[P, P] - Fr[P, P]) <= 1e-10 * Fr[P, P]
    out = chain.getRegressorGramWide(*ts)
    first = [t.clone() for t in out]
    chain.getRegressorGramWide(*ts, out=out, accumulate=True)
    assert all(_fro(x.cpu().numpy(), 2 * y.cpu().numpy()) <= 1e-15 for x, y in zip(out, first))
    # without tau_meas: c = 0, bb = 0
    G0, c0, bb0 = chain.getRegressorGramWide(*ts[:3])
    assert torch.equal(G0, first[0]) and not c0.abs().max().item() and not bb0.abs().max().item()
    # N = 0: zeros, or the outputs left alone when accumulating
    empty = [x[:0].contiguous() for x in ts]
    Gz, cz, bbz = chain.getRegressorGramWide(*empty)
    assert not Gz.abs().max().item() and not cz.abs().max().item() and not bbz.abs().max().item()
    chain.getRegressorGramWide(*empty, out=out, accumulate=True)
    assert all(_fro(x.cpu().numpy(), 2 * y.cpu().numpy()) <= 1e-15 for x, y in zip(out, first))


@pytest.mark.parametrize("case", ["rev14_mixed", "ur6_26_friction"])
def test_identification_gram_wide_matches_oracle(case):
    """[Y | C] from the oracle's regressor and components_regressor: a 14-joint chain with FRICTION1, FRICTION2 and SPRING components
    on several joints (140 + 16 columns), and the 6-joint UR with 26 friction models (60 + 52 columns, refused by the narrow call)."""
    torch = pytest.importorskip("torch")
    from oracle.oracle import components_regressor
    from rosdyn_amd.components import ComponentSet
    from rosdyn_amd.samples import trajectory_batch
    if case == "ur6_26_friction":
        chain, ref = _ur6()
        specs = [(0, j % 6, 1e-3, 5.0, [0.4 + 0.01 * j, 1.0 + 0.02 * j]) for j in range(26)]
    else:
        chain, ref = _chain_case("rev14")
        specs = [(0, 0, 1e-3, 5.0, [0.4, 1.0]), (1, 3, 1e-3, 4.0, [0.3, 0.7, 0.05]), (2, 5, 0.0, 0.0, [2.0, 0.1]),
                 (0, 9, 1e-3, 5.0, [0.2, 0.6]), (1, 13, 1e-3, 3.0, [0.25, 0.5, 0.02]), (2, 13, 0.0, 0.0, [1.5, -0.2])]
    n, P, N = ref.n, ref.P, 700
    comps = ComponentSet([dict(type=sp[0], joint=sp[1], min_velocity=sp[2], max_velocity=sp[3], parameters=sp[4]) for sp in specs], n)
    K = comps.columns
    q, dq, ddq = trajectory_batch(17, N, n)
    Cm, tau_c = components_regressor(specs, n, q, dq)
    tau = ref.joint_torque(q, dq, ddq) + tau_c + 1e-3 * np.random.default_rng(4).normal(size=(N, n))
    M = np.column_stack([ref.regressor(q, dq, ddq).reshape(N * n, P), Cm.reshape(N * n, K), tau.reshape(-1)])
    Fr = M.T @ M
    ts = [torch.from_numpy(x).cuda() for x in (q, dq, ddq, tau)]
    te = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in (q, dq, ddq, tau)]
    for args, layout, chunk in ((ts, "sample", 0), (te, "element", 0), (ts, "sample", 160)):
        F = _full(*chain.getIdentificationGramWide(comps, *args, layout=layout, chunk_samples=chunk))
        assert F.shape == (P + K + 1, P + K + 1)
        assert _fro(F, Fr) <= 1e-10, (layout, chunk)


def test_identification_end_to_end_fourteen_joints():
    """tau = Y pi + C theta + 1e-9 noise on a 14-joint chain -> wide normal equations -> rdyn_solve_normal_equations: the torques of
    1 000 fresh samples are predicted and the friction coefficients recovered."""
    torch = pytest.importorskip("torch")
    from oracle.oracle import components_regressor
    from rosdyn_amd.components import ComponentSet
    from rosdyn_amd.gram import solve_normal_equations_abi
    from rosdyn_amd.samples import trajectory_batch
    chain, ref = _chain_case("rev14")
    n, P, N = 14, 140, 4000
    specs = [(0, j, 1e-3, 5.0, [0.3 + 0.05 * j, 0.8 + 0.1 * j]) for j in (0, 3, 7, 13)] + \
            [(1, j, 1e-3, 5.0, [0.2 + 0.05 * j, 0.5, 0.05]) for j in (1, 9, 12)]
    theta = np.concatenate([np.array(sp[4][:3 if sp[0] == 1 else 2]) for sp in specs])
    comps = ComponentSet([dict(type=sp[0], joint=sp[1], min_velocity=sp[2], max_velocity=sp[3], parameters=sp[4]) for sp in specs], n)
    pi = ref.nominal_parameters()
    q, dq, ddq = trajectory_batch(91, N, n)
    _, tau_c = components_regressor(specs, n, q, dq)
    tau = ref.joint_torque(q, dq, ddq) + tau_c + 1e-9 * np.random.default_rng(5).normal(size=(N, n))
    G, c, _ = chain.getIdentificationGramWide(comps, *(torch.from_numpy(x).cuda() for x in (q, dq, ddq, tau)))
    x, rank = solve_normal_equations_abi(G, c)
    assert 0 < rank < P + comps.columns
    assert np.abs(x[P:] - theta).max() <= 1e-6 * np.abs(theta).max()
    q2, dq2, ddq2 = trajectory_batch(191, 1000, n)
    C2, tc2 = components_regressor(specs, n, q2, dq2)
    Y2 = ref.regressor(q2, dq2, ddq2)
    true = np.einsum("snp,p->sn", Y2, pi) + tc2
    pred = np.einsum("snp,p->sn", Y2, x[:P]) + np.einsum("snk,k->sn", C2, x[P:])
    assert np.linalg.norm(pred - true) <= 1e-6 * np.linalg.norm(true)


@pytest.mark.parametrize("case", ["ur6", "ur_tool0", "rev11"])
def test_wide_calls_match_narrow_calls_where_both_serve(case):
    """Requests the narrow calls already serve: the wide call hands them over (UR 6 joints, UR to tool0 through the reduced companion,
    11 revolute input joints through the long chunk images)."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd import Chain
    from rosdyn_amd.components import ComponentSet
    from rosdyn_amd.samples import trajectory_batch
    if case == "rev11":
        chain = Chain(generated_revolute_chain(11, 1111), "l0", "l11", GRAV)
    else:
        path = os.path.join(FIXTURES, "ur10_like.urdf")
        chain = Chain(path, "base_link", "wrist_3_link" if case == "ur6" else "tool0", GRAV)
    n, N = chain.getActiveJointsNumber(), 1500
    q, dq, ddq, tau = trajectory_batch(29, N, n, order=4)
    args = [torch.from_numpy(x).cuda() for x in (q, dq, ddq, tau)]
    Fn = _full(*chain.getRegressorGram(*args))
    Fw = _full(*chain.getRegressorGramWide(*args))
    assert _fro(Fw, Fn) <= 1e-12
    if case != "rev11":
        comps = ComponentSet([dict(type=j % 3, joint=j, min_velocity=1e-3, max_velocity=5.0, parameters=[0.3, 0.5, 0.1]) for j in range(n)], n)
        Fn = _full(*chain.getIdentificationGram(comps, *args))
        Fw = _full(*chain.getIdentificationGramWide(comps, *args))
        assert _fro(Fw, Fn) <= 1e-12


def test_regressor_gram_wide_replays_from_a_graph():
    """One single-stream capture of getRegressorGramWide on the 20-joint chain: the replay gives the eager call's bits."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd._lib import lib
    chain, _ = _chain_case("rev20")
    n, P, N = 20, 200, 3000
    q, dq, ddq, tau = (torch.rand((N, n), dtype=torch.float64, device="cuda") * 2 - 1 for _ in range(4))
    out = (torch.empty((P, P), dtype=torch.float64, device="cuda"), torch.empty((P,), dtype=torch.float64, device="cuda"),
           torch.empty((1,), dtype=torch.float64, device="cuda"))
    ws = torch.empty((lib().rdyn_regressor_gram_wide_workspace_bytes(chain._h, 1024),), dtype=torch.uint8, device="cuda")
    chain.getRegressorGramWide(q, dq, ddq, tau, chunk_samples=1024, out=out, workspace=ws)   # first use uploads the chain constants
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            chain.getRegressorGramWide(q, dq, ddq, tau, chunk_samples=1024, out=out, workspace=ws)
    q.uniform_(-1, 1)                       # new inputs, same buffers
    out[0].zero_()
    g.replay()
    torch.cuda.synchronize()
    G2, c2, bb2 = chain.getRegressorGramWide(q, dq, ddq, tau, chunk_samples=1024)
    assert torch.equal(out[0], G2) and torch.equal(out[1], c2) and torch.equal(out[2], bb2)
