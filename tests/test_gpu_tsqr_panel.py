"""GPU tests of the R factors wider than 112 columns: the column-panel CholeskyQR (rdyn_panel_trmm.hip, rdyn_panel_gram.hip and the
PANEL dense steps of rdyn_cholqr.hip) behind rdyn_tsqr_wide, rdyn_regressor_tsqr_wide and rdyn_identification_tsqr_wide, against numpy
and the C oracle."""
import numpy as np
import pytest

from _chains import WIDE_GRAV as GRAV, _chain_case, _ur6

pytestmark = pytest.mark.gpu


def _fro(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _gram_of(R):
    R = R.cpu().numpy() if hasattr(R, "cpu") else R
    return R.T @ R


def _is_upper(R):
    R = R.cpu().numpy()
    return not np.tril(R, -1).any()


@pytest.mark.parametrize("n_cols", [113, 200, 321, 415])
@pytest.mark.parametrize("with_b", [True, False])
def test_tsqr_wide_matches_numpy(n_cols, with_b):
    """rdyn_tsqr_wide on seeded random matrices: R'R = M'M, |R| = |qr(M).R| row by row, ragged rows and lda > rows, accumulate,
    bitwise reproducible."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.gram import tsqr_wide, tsqr_wide_last_report
    from rosdyn_amd._lib import lib
    rng = np.random.default_rng(2000 + n_cols)
    for rows, lda in ((3001, 3001), (1237, 1250)):
        Ah = rng.normal(size=(n_cols, lda))
        bh = rng.normal(size=rows) if with_b else None
        A = torch.from_numpy(Ah).cuda()
        b = torch.from_numpy(bh).cuda() if with_b else None
        n1 = n_cols + (1 if with_b else 0)
        ws = torch.empty((lib().rdyn_tsqr_wide_workspace_bytes(n1),), dtype=torch.uint8, device="cuda")
        R = tsqr_wide(A, b, rows=rows, workspace=ws)
        assert R.shape == (n1, n1) and _is_upper(R)
        M = Ah[:, :rows].T if not with_b else np.column_stack([Ah[:, :rows].T, bh])
        F = M.T @ M
        assert _fro(_gram_of(R), F) <= 1e-12, (rows, lda)
        Rn = np.linalg.qr(M, mode="r")
        Rh = R.cpu().numpy()
        assert np.abs(np.abs(Rh) - np.abs(Rn)).max() <= 1e-10 * np.abs(Rn).max()
        rep = tsqr_wide_last_report(n1, ws)
        assert rep["route"] == 2 and rep["stage"] < 3, rep
        R2 = tsqr_wide(A, b, rows=rows, workspace=ws)
        assert torch.equal(R, R2)
        out = R.clone()
        tsqr_wide(A, b, rows=rows, out=out, accumulate=True, workspace=ws)
        assert _is_upper(out) and _fro(_gram_of(out), 2 * F) <= 1e-12


def test_tsqr_wide_keeps_the_digits_the_normal_equations_lose():
    """200 columns, 65 536 rows, cond(A) = 1e9: R'R = M'M, the R route recovers x to 1e-4 and the normal equations of the same problem
    are >= 100x worse.  (No round meets rho <= 4 here -- the preconditioner defers the pivots below 1e-5 of their column -- so the
    report says stage 3, and the factor that stands is still the accurate one.)"""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.gram import gram_wide, solve_normal_equations_abi, solve_r_factor, tsqr_wide, tsqr_wide_last_report
    from rosdyn_amd._lib import lib
    rng = np.random.default_rng(77)
    rows, n = 65536, 200
    U, _ = np.linalg.qr(rng.normal(size=(rows, n)))
    V, _ = np.linalg.qr(rng.normal(size=(n, n)))
    Ah = (U * np.logspace(0, -9, n)) @ V.T
    x = rng.normal(size=n)
    bh = Ah @ x
    A = torch.from_numpy(np.ascontiguousarray(Ah.T)).cuda()
    b = torch.from_numpy(bh).cuda()
    ws = torch.empty((lib().rdyn_tsqr_wide_workspace_bytes(n + 1),), dtype=torch.uint8, device="cuda")
    R = tsqr_wide(A, b, workspace=ws)
    rep = tsqr_wide_last_report(n + 1, ws)
    assert rep["route"] == 2 and 0 <= rep["stage"] <= 3 and rep["gamma"][0] > 0, rep
    M = np.column_stack([Ah, bh])
    assert _fro(_gram_of(R), M.T @ M) <= 1e-12
    xr, _ = solve_r_factor(R, n, rtol=1e-14)
    err_r = np.linalg.norm(xr - x) / np.linalg.norm(x)
    G, c, _ = gram_wide(A, b)
    xn, _ = solve_normal_equations_abi(G, c)
    err_n = np.linalg.norm(xn - x) / np.linalg.norm(x)
    assert err_r <= 1e-4, err_r
    assert err_n >= 100 * err_r, (err_n, err_r)


@pytest.mark.parametrize("n_cols", [60, 111])
def test_tsqr_wide_hands_narrow_widths_to_rdyn_tsqr(n_cols):
    """A width rdyn_tsqr serves: the wide call returns its result (same workspace size) and the report says route 0."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.gram import tsqr, tsqr_wide, tsqr_wide_last_report
    from rosdyn_amd._lib import lib
    assert lib().rdyn_tsqr_wide_workspace_bytes(n_cols + 1) == lib().rdyn_tsqr_workspace_bytes(n_cols + 1)
    rng = np.random.default_rng(n_cols)
    A = torch.from_numpy(rng.normal(size=(n_cols, 40000))).cuda()
    b = torch.from_numpy(rng.normal(size=40000)).cuda()
    Rn = tsqr(A, b)
    ws = torch.empty((lib().rdyn_tsqr_wide_workspace_bytes(n_cols + 1),), dtype=torch.uint8, device="cuda")
    Rw = tsqr_wide(A, b, workspace=ws)
    assert _fro(Rw.cpu().numpy(), Rn.cpu().numpy()) <= 1e-13
    assert tsqr_wide_last_report(n_cols + 1, ws)["route"] == 0


def test_tsqr_wide_replays_in_a_graph():
    """rdyn_tsqr_wide captured in a torch.cuda.graph (several row chunks, all three rounds queued) and replayed equals the eager result
    bitwise."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.gram import tsqr_wide
    from rosdyn_amd._lib import lib
    n_cols, rows = 300, 120000
    rng = np.random.default_rng(9)
    A = torch.from_numpy(rng.normal(size=(n_cols, rows))).cuda()
    b = torch.from_numpy(rng.normal(size=rows)).cuda()
    ws = torch.empty((lib().rdyn_tsqr_wide_workspace_bytes(n_cols + 1),), dtype=torch.uint8, device="cuda")
    eager = tsqr_wide(A, b, workspace=ws).clone()
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tsqr_wide(A, b, out=out, workspace=ws)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tsqr_wide(A, b, out=out, workspace=ws)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_tsqr_wide_subsampled_preconditioner():
    """300 columns x 300 000 rows: the preconditioner comes from every S-th 16-row group (S > 1) and the rows run in several chunks;
    R'R = M'M and |R| = |qr(M).R| row by row."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.gram import tsqr_wide, tsqr_wide_last_report
    from rosdyn_amd._lib import lib
    n_cols, rows = 300, 300000
    rng = np.random.default_rng(300)
    scales = np.logspace(0, 3, n_cols)
    Ah = rng.normal(size=(n_cols, rows)) * scales[:, None]
    bh = rng.normal(size=rows)
    A = torch.from_numpy(Ah).cuda()
    b = torch.from_numpy(bh).cuda()
    ws = torch.empty((lib().rdyn_tsqr_wide_workspace_bytes(n_cols + 1),), dtype=torch.uint8, device="cuda")
    R = tsqr_wide(A, b, workspace=ws)
    rep = tsqr_wide_last_report(n_cols + 1, ws)
    assert rep["route"] == 2 and rep["stage"] < 3, rep
    assert _is_upper(R)
    At = torch.cat([A, b.view(1, -1)]).t()
    F = (At.t() @ At).cpu().numpy()
    assert _fro(_gram_of(R), F) <= 1e-12
    Rn = np.linalg.qr(At.cpu().numpy(), mode="r")
    Rh = R.cpu().numpy()
    assert np.abs(np.abs(Rh) - np.abs(Rn)).max() <= 1e-10 * np.abs(Rn).max()


def test_tsqr_wide_rank_deficient_columns_give_zero_rows():
    """200 columns of which 40 beyond column 128 are exact multiples (x2) of earlier ones: those rows of R are exactly zero and R'R = M'M."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.gram import tsqr_wide, tsqr_wide_last_report
    from rosdyn_amd._lib import lib
    n_cols, rows = 200, 300000
    rng = np.random.default_rng(201)
    Ah = rng.normal(size=(n_cols, rows))
    dep = list(range(140, 180))
    for k in dep:
        Ah[k] = 2.0 * Ah[k - 120]
    bh = rng.normal(size=rows)
    A = torch.from_numpy(Ah).cuda()
    b = torch.from_numpy(bh).cuda()
    ws = torch.empty((lib().rdyn_tsqr_wide_workspace_bytes(n_cols + 1),), dtype=torch.uint8, device="cuda")
    R = tsqr_wide(A, b, workspace=ws)
    rep = tsqr_wide_last_report(n_cols + 1, ws)
    assert rep["route"] == 2 and rep["stage"] < 3, rep
    Rh = R.cpu().numpy()
    zero = [k for k in range(n_cols + 1) if not np.abs(Rh[k]).max()]
    assert zero == dep
    M = np.column_stack([Ah.T, bh])
    assert _fro(Rh.T @ Rh, M.T @ M) <= 1e-12


@pytest.mark.parametrize("case", ["rev12", "rev14", "rev20", "rev32", "gen20_twelve_permuted"])
def test_regressor_tsqr_wide_matches_oracle(case):
    """R'R = F (the oracle Gram of [Y | tau]) for chains of 12 to 32 input joints, both layouts, default and ragged chunks, accumulate,
    tau_meas = None, N = 0, and a batch with fewer rows than columns."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.samples import trajectory_batch
    chain, ref = _chain_case(case)
    n, P, N = ref.n, ref.P, 250
    q, dq, ddq = trajectory_batch(81, N, n)
    tau = ref.joint_torque(q, dq, ddq) + 1e-3 * np.random.default_rng(3).normal(size=(N, n))
    M = np.column_stack([ref.regressor(q, dq, ddq).reshape(N * n, P), tau.reshape(-1)])
    Fr = M.T @ M
    ts = [torch.from_numpy(x).cuda() for x in (q, dq, ddq, tau)]
    te = [torch.from_numpy(np.ascontiguousarray(x.T)).cuda() for x in (q, dq, ddq, tau)]
    for args, layout in ((ts, "sample"), (te, "element")):
        for chunk in (0, 96):
            R = chain.getRegressorTsqrWide(*args, layout=layout, chunk_samples=chunk)
            assert R.shape == (P + 1, P + 1) and _is_upper(R)
            assert _fro(_gram_of(R), Fr) <= 1e-10, (layout, chunk)
    ws = torch.empty((_chain_ws(chain),), dtype=torch.uint8, device="cuda")
    R = chain.getRegressorTsqrWide(*ts, workspace=ws)
    rep = chain.lastTsqrWideReport(ws)
    assert rep["route"] == 2 and 0 <= rep["stage"] <= 3 and rep["n_deferred"] > 0, rep
    assert torch.equal(R, chain.getRegressorTsqrWide(*ts, workspace=ws))
    out = R.clone()
    chain.getRegressorTsqrWide(*ts, out=out, accumulate=True)
    assert _fro(_gram_of(out), 2 * Fr) <= 1e-10
    F0 = _gram_of(chain.getRegressorTsqrWide(*ts[:3]))
    assert _fro(F0[:P, :P], Fr[:P, :P]) <= 1e-10 and not np.abs(F0[:, P]).max()
    empty = [x[:0].contiguous() for x in ts]
    assert not chain.getRegressorTsqrWide(*empty).abs().max().item()
    chain.getRegressorTsqrWide(*empty, out=out, accumulate=True)
    assert _fro(_gram_of(out), 2 * Fr) <= 1e-10
    if n == 32:
        q4, dq4, ddq4, t4 = (np.ascontiguousarray(x[:4]) for x in (q, dq, ddq, tau))
        M4 = np.column_stack([ref.regressor(q4, dq4, ddq4).reshape(4 * n, P), t4.reshape(-1)])
        R4 = chain.getRegressorTsqrWide(*(torch.from_numpy(x).cuda() for x in (q4, dq4, ddq4, t4)))
        # 128 rows for 321 columns: rank <= 128, no round is accepted (stage 3); measured 1.7e-8
        assert _is_upper(R4) and _fro(_gram_of(R4), M4.T @ M4) <= 1e-7


def _chain_ws(chain, comps=None):
    import ctypes as C
    from rosdyn_amd._lib import lib
    if comps is None:
        return lib().rdyn_regressor_tsqr_wide_workspace_bytes(chain._h, 0)
    return lib().rdyn_identification_tsqr_wide_workspace_bytes(chain._h, C.cast(comps._arr, C.c_void_p), comps.n_comps, 0)


@pytest.mark.parametrize("case", ["rev14_mixed", "ur6_26_friction"])
def test_identification_tsqr_wide_matches_oracle(case):
    """[Y | C | tau]: a 14-joint chain with mixed components, and the 6-joint UR with 26 friction models (through the reduced
    companion): R'R = F."""
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
        R = chain.getIdentificationTsqrWide(comps, *args, layout=layout, chunk_samples=chunk)
        assert R.shape == (P + K + 1, P + K + 1) and _is_upper(R)
        assert _fro(_gram_of(R), Fr) <= 1e-10, (layout, chunk)
    ws = torch.empty((_chain_ws(chain, comps),), dtype=torch.uint8, device="cuda")
    chain.getIdentificationTsqrWide(comps, *ts, workspace=ws)
    rep = chain.lastTsqrWideReport(ws, comps)
    assert rep["route"] == 2 and 0 <= rep["stage"] <= 3, rep


def test_identification_tsqr_wide_end_to_end_fourteen_joints():
    """tau = Y pi + C theta + 1e-9 noise on a 14-joint chain -> wide R factor -> rdyn_solve_r_factor: the friction coefficients are
    recovered and the torques of 1 000 fresh samples predicted."""
    torch = pytest.importorskip("torch")
    from oracle.oracle import components_regressor
    from rosdyn_amd.components import ComponentSet
    from rosdyn_amd.gram import solve_r_factor
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
    R = chain.getIdentificationTsqrWide(comps, *(torch.from_numpy(x).cuda() for x in (q, dq, ddq, tau)))
    x, rank = solve_r_factor(R, P + comps.columns)
    assert 0 < rank < P + comps.columns
    assert np.abs(x[P:] - theta).max() <= 1e-6 * np.abs(theta).max()
    q2, dq2, ddq2 = trajectory_batch(191, 1000, n)
    C2, tc2 = components_regressor(specs, n, q2, dq2)
    Y2 = ref.regressor(q2, dq2, ddq2)
    true = np.einsum("snp,p->sn", Y2, pi) + tc2
    pred = np.einsum("snp,p->sn", Y2, x[:P]) + np.einsum("snk,k->sn", C2, x[P:])
    assert np.linalg.norm(pred - true) <= 1e-6 * np.linalg.norm(true)


@pytest.mark.parametrize("case", ["ur6", "ur_tool0", "rev11"])
def test_regressor_tsqr_wide_hands_narrow_chains_to_the_narrow_call(case):
    """Where the narrow call serves, the wide call returns its result."""
    torch = pytest.importorskip("torch")
    import os
    from conftest import FIXTURES
    from oracle.oracle import OracleChain
    from rosdyn_amd import Chain
    from rosdyn_amd.samples import trajectory_batch
    if case == "ur6":
        chain, ref = _ur6()
    elif case == "ur_tool0":
        path = os.path.join(FIXTURES, "ur10_like.urdf")
        chain, ref = Chain(path, "base_link", "tool0", GRAV), OracleChain(path, "base_link", "tool0", GRAV)
    else:
        chain, ref = _chain_case("rev11")
    n, N = chain.getActiveJointsNumber(), 300
    q, dq, ddq = trajectory_batch(5, N, n)
    ts = [torch.from_numpy(x).cuda() for x in (q, dq, ddq, ref.joint_torque(q, dq, ddq))]
    assert _fro(chain.getRegressorTsqrWide(*ts).cpu().numpy(), chain.getRegressorTsqr(*ts).cpu().numpy()) <= 1e-13


def test_regressor_tsqr_wide_replays_in_a_graph():
    """getRegressorTsqrWide captured in a torch.cuda.graph and replayed equals the eager result bitwise."""
    torch = pytest.importorskip("torch")
    from rosdyn_amd.samples import trajectory_batch
    chain, ref = _chain_case("rev14")
    n, N = ref.n, 2000
    q, dq, ddq = trajectory_batch(33, N, n)
    ts = [torch.from_numpy(x).cuda() for x in (q, dq, ddq, ref.joint_torque(q, dq, ddq))]
    ws = torch.empty((_chain_ws(chain),), dtype=torch.uint8, device="cuda")
    eager = chain.getRegressorTsqrWide(*ts, workspace=ws).clone()
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain.getRegressorTsqrWide(*ts, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain.getRegressorTsqrWide(*ts, out=out, workspace=ws)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
