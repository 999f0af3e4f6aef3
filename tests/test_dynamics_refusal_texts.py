"""CPU tests (no GPU): the exact rdyn_last_error() text of every refusal the seven entries of the forward-dynamics family and
rdyn_joint_torque_derivatives make before they touch a device, and which refusal wins when a call has two faults.  The texts are the
library's, written out literally: a refusal that changes its wording or its place in the order of the checks fails here.
(The one refusal these entries make AFTER entering the device -- the per-joint state that exceeds the LDS -- cannot be reached without
one and is not covered.)  Nothing here touches a device: every call fails its checks first; fake pointers are never dereferenced."""
import ctypes as C

import pytest

from _cabi import FAKE, _chain, _comp

INVALID = 1
N = 7
CHAINS = ["ur10_like", "rev11"]   # one chain swept in registers (no workspace), one on the chunked route
CHUNKED = {"rev11"}

T_INTEGRATOR = "negative n_steps, a step size that is zero or not finite, or an unknown integrator"
T_COMPONENT_LIST = "0..30 components, a list when there are any"
T_BAD_COMPONENT = "component 0 has an invalid type or joint"     # (no entry name: the component check's own text)
T_MISMATCH = "Input data dimensions mismatch"                    # (no entry name: the reference's text)


def _rollout_desc(n, **kw):
    from rosdyn_amd._lib import RolloutDesc
    d = RolloutDesc()
    d.n_steps, d.integrator, d.dt = 5, 1, 1e-3
    d.tau, d.tau_step_stride = FAKE, n * N
    d.q_end, d.dq_end, d.q_traj, d.dq_traj = FAKE, FAKE, None, None
    d.traj_step_stride, d.traj_every = 0, 0
    d.status = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _adjoint_desc(n, **kw):
    from rosdyn_amd._lib import RolloutAdjointDesc
    d = RolloutAdjointDesc()
    d.n_steps, d.integrator, d.dt = 5, 1, 1e-3
    d.tau, d.tau_step_stride = FAKE, n * N
    d.q_traj, d.dq_traj, d.traj_step_stride = FAKE, FAKE, n * N
    d.gq_end, d.gdq_end = FAKE, FAKE
    d.gq_traj, d.gdq_traj, d.gtraj_step_stride = FAKE, FAKE, n * N
    d.gq0, d.gdq0, d.gtau, d.gtau_step_stride = FAKE, FAKE, FAKE, n * N
    d.status = FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


class Entry:
    """One entry point: `who` (the name in its texts), whether it takes a descriptor / components, its pointer arguments (name -> default)
    in the order of the C signature between the component list and chunk_samples, and its workspace query."""

    def __init__(self, who, desc=None, comps=False, pointers=(), query=None, workspace=True):
        self.who, self.desc, self.comps, self.pointers, self.query, self.workspace = who, desc, comps, pointers, query, workspace

    def need(self, chain, d, chunk_samples):
        from rosdyn_amd._lib import lib
        if not self.workspace:
            return 0
        q = getattr(lib(), self.query)
        return q(chain._h, C.byref(d), N, chunk_samples) if self.desc else q(chain._h, chunk_samples)

    def call(self, chain, n_samples=N, batch=True, q=FAKE, dq=FAKE, ddq_in=FAKE, layout=0, desc=True, comps=None, n_comps=0, chunk_samples=0,
             workspace=FAKE, short=None, **kw):
        """Returns (return code, last error text).  short: bytes missing from the workspace size the query asks for.  The other keywords
        override a pointer argument or a descriptor field."""
        from rosdyn_amd._lib import Batch, lib
        b = Batch()
        b.n_samples, b.q, b.dq, b.ddq, b.layout, b.device = n_samples, q, dq, ddq_in, layout, 0
        n = chain.getActiveJointsNumber()
        args = [chain._h, C.byref(b) if batch else None]
        d = None
        if self.desc:
            fields = {k: kw.pop(k) for k in list(kw) if k not in self.pointers}
            d = (_rollout_desc if self.desc == "rollout" else _adjoint_desc)(n, **fields)
            args.append(C.byref(d) if desc else None)
        if self.comps:
            args += [comps, n_comps]
        args += [kw.pop(name, FAKE) for name in self.pointers]
        assert not kw, kw
        if self.workspace:
            need = self.need(chain, d, max(chunk_samples, 0))
            args += [chunk_samples, workspace, max(need - (short or 0), 0)]
        rc = getattr(lib(), self.who)(*args)
        return rc, lib().rdyn_last_error().decode()


FD = Entry("rdyn_forward_dynamics", pointers=("tau", "ddq", "status"), query="rdyn_forward_dynamics_workspace_bytes")
FDC = Entry("rdyn_forward_dynamics_components", comps=True, pointers=("tau", "ddq", "status"), query="rdyn_forward_dynamics_workspace_bytes")
RO = Entry("rdyn_rollout", desc="rollout", query="rdyn_rollout_workspace_bytes")
ROC = Entry("rdyn_rollout_components", desc="rollout", comps=True, query="rdyn_rollout_workspace_bytes")
FDD = Entry("rdyn_forward_dynamics_derivatives", comps=True, pointers=("tau", "ddq", "dddq_dq", "dddq_dv", "minv", "status"),
            query="rdyn_forward_dynamics_derivatives_workspace_bytes")
VJP = Entry("rdyn_forward_dynamics_vjp", comps=True, pointers=("tau", "ddq_bar", "q_bar", "dq_bar", "tau_bar", "ddq", "status"),
            query="rdyn_forward_dynamics_vjp_workspace_bytes")
ADJ = Entry("rdyn_rollout_adjoint", desc="adjoint", comps=True, query="rdyn_rollout_adjoint_workspace_bytes")
JTD = Entry("rdyn_joint_torque_derivatives", pointers=("dtau_dq", "dtau_dv", "M"), workspace=False)
ENTRIES = [FD, FDC, RO, ROC, FDD, VJP, ADJ, JTD]

# the refusals of an entry beyond those all share: (keywords of the faulty call, text behind "<who>: ")
OWN = {
    FD.who: [({"tau": None}, "null torque or acceleration pointer"), ({"ddq": None}, "null torque or acceleration pointer")],
    FDC.who: [({"tau": None}, "null torque or acceleration pointer"), ({"ddq": None}, "null torque or acceleration pointer")],
    FDD.who: [({"tau": None}, "null torque or acceleration pointer"), ({"ddq": None}, "null torque or acceleration pointer"),
              ({"dddq_dq": None, "dddq_dv": None, "minv": None}, "every matrix output is null")],
    VJP.who: [({"tau": None}, "null torque or seed pointer"), ({"ddq_bar": None}, "null torque or seed pointer"),
              ({"q_bar": None, "dq_bar": None, "tau_bar": None}, "every product is null")],
    JTD.who: [({"dtau_dq": None, "dtau_dv": None, "M": None}, "every output is null")],
}
ROLLOUT_OWN = [
    ({"desc": False}, "null descriptor"),
    ({"n_steps": -1}, T_INTEGRATOR), ({"dt": 0.0}, T_INTEGRATOR), ({"dt": float("nan")}, T_INTEGRATOR), ({"dt": float("inf")}, T_INTEGRATOR),
    ({"integrator": 2}, T_INTEGRATOR), ({"integrator": -1}, T_INTEGRATOR),
    ({"tau": None}, "null torque pointer"),
    ({"q_end": None, "dq_end": None}, "every output is null"),
    ({"q_traj": FAKE, "traj_every": 0, "traj_step_stride": 1 << 20}, "a trajectory needs traj_every >= 1 and traj_step_stride >= n * n_samples"),
    ({"dq_traj": FAKE, "traj_every": 1, "traj_step_stride": 0}, "a trajectory needs traj_every >= 1 and traj_step_stride >= n * n_samples"),
]
OWN[RO.who] = OWN[ROC.who] = ROLLOUT_OWN
T_ADJ_STRIDES = "traj_step_stride, gtraj_step_stride and a non-zero gtau_step_stride must be >= n * n_samples"
OWN[ADJ.who] = [
    ({"desc": False}, "null descriptor"),
    ({"n_steps": -1}, T_INTEGRATOR), ({"dt": 0.0}, T_INTEGRATOR), ({"dt": float("nan")}, T_INTEGRATOR), ({"integrator": 2}, T_INTEGRATOR),
    ({"tau": None}, "null torque pointer"),
    ({"q_traj": None}, "two or more steps need the forward call's trajectory (q_traj and dq_traj, traj_every = 1)"),
    ({"dq_traj": None}, "two or more steps need the forward call's trajectory (q_traj and dq_traj, traj_every = 1)"),
    ({"traj_step_stride": 0}, T_ADJ_STRIDES), ({"gtraj_step_stride": 1}, T_ADJ_STRIDES), ({"gtau_step_stride": 1}, T_ADJ_STRIDES),
    ({"gq0": None, "gdq0": None, "gtau": None}, "every output is null"),
]


def _refused(entry, chain, text, **kw):
    rc, msg = entry.call(chain, **kw)
    assert rc == INVALID, (entry.who, kw, rc, msg)
    assert msg == text, (entry.who, kw)


@pytest.fixture(scope="module", params=CHAINS)
def chain(request):
    c = _chain(request.param)
    c.name = request.param
    return c


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.who)
def test_every_refusal_has_its_text(chain, entry):
    who = entry.who
    # the batch checks every entry shares
    _refused(entry, chain, who + ": null chain or batch", batch=False)
    _refused(entry, chain, who + ": invalid n_samples or layout", n_samples=-1)
    _refused(entry, chain, who + ": invalid n_samples or layout", layout=5)
    _refused(entry, chain, T_MISMATCH, q=None)
    _refused(entry, chain, T_MISMATCH, dq=None)
    if entry is JTD:
        _refused(entry, chain, T_MISMATCH, ddq_in=None)
    for kw, text in OWN[who]:
        _refused(entry, chain, who + ": " + text, **kw)
    if not entry.workspace:
        return
    _refused(entry, chain, who + ": negative chunk_samples", chunk_samples=-1)
    _refused(entry, chain, who + ": negative chunk_samples", chunk_samples=-64, n_samples=0)
    if chain.name in CHUNKED:
        for chunk in (0, 1000):
            need = entry.need(chain, (_rollout_desc if entry.desc == "rollout" else _adjoint_desc)(chain.getActiveJointsNumber()) if entry.desc
                              else None, chunk)
            assert need > 1
            _refused(entry, chain, "%s: workspace too small (%d < %d bytes)" % (who, need - 1, need), chunk_samples=chunk, short=1)
            _refused(entry, chain, "%s: workspace too small (0 < %d bytes)" % (who, need), chunk_samples=chunk, workspace=None)
    if entry.comps:
        one, bad_type, bad_joint = _comp(), _comp(ctype=77), _comp(joint=chain.getActiveJointsNumber())
        _refused(entry, chain, who + ": " + T_COMPONENT_LIST, comps=None, n_comps=1)
        _refused(entry, chain, who + ": " + T_COMPONENT_LIST, comps=C.addressof(one), n_comps=-1)
        _refused(entry, chain, who + ": " + T_COMPONENT_LIST, comps=C.addressof(one), n_comps=31)
        _refused(entry, chain, T_BAD_COMPONENT, comps=C.addressof(bad_type), n_comps=1)
        _refused(entry, chain, T_BAD_COMPONENT, comps=C.addressof(bad_joint), n_comps=1)
        _refused(entry, chain, T_BAD_COMPONENT, comps=C.addressof(bad_type), n_comps=1, n_samples=0)


NULL_TAU_TEXT = {FD.who: "null torque or acceleration pointer", FDC.who: "null torque or acceleration pointer",
                 FDD.who: "null torque or acceleration pointer", VJP.who: "null torque or seed pointer",
                 RO.who: "null torque pointer", ROC.who: "null torque pointer", ADJ.who: "null torque pointer"}


@pytest.mark.parametrize("entry", ENTRIES[:-1], ids=lambda e: e.who)
def test_which_refusal_wins(chain, entry):
    who = entry.who
    # a null tau with a negative chunk_samples: the pointer check
    _refused(entry, chain, who + ": " + NULL_TAU_TEXT[who], tau=None, chunk_samples=-1)
    # a negative chunk_samples with a short workspace: the chunk's sign
    _refused(entry, chain, who + ": negative chunk_samples", chunk_samples=-1, short=1)
    _refused(entry, chain, who + ": negative chunk_samples", chunk_samples=-1, workspace=None)
    if entry.comps:
        # a short workspace with a bad component type: the workspace where the chain needs one, else the component
        bad_type = _comp(ctype=77)
        if chain.name in CHUNKED:
            rc, msg = entry.call(chain, comps=C.addressof(bad_type), n_comps=1, short=1)
            assert rc == INVALID and msg.startswith(who + ": workspace too small ("), msg
            rc, msg = entry.call(chain, comps=None, n_comps=1, workspace=None)
            assert rc == INVALID and msg.startswith(who + ": workspace too small (0 < "), msg
        else:
            _refused(entry, chain, T_BAD_COMPONENT, comps=C.addressof(bad_type), n_comps=1, short=1)
        # a negative chunk_samples with a bad component: the chunk's sign
        _refused(entry, chain, who + ": negative chunk_samples", comps=C.addressof(bad_type), n_comps=1, chunk_samples=-1)
    if entry.desc:
        # a null descriptor with a null batch: the batch; a bad integrator with a null tau: the integrator
        _refused(entry, chain, who + ": null chain or batch", desc=False, batch=False)
        _refused(entry, chain, who + ": " + T_INTEGRATOR, integrator=7, tau=None)
        _refused(entry, chain, who + ": null descriptor", desc=False, chunk_samples=-1)
        # every output null with a negative chunk_samples: the outputs
        outs = {"q_end": None, "dq_end": None} if entry.desc == "rollout" else {"gq0": None, "gdq0": None, "gtau": None}
        _refused(entry, chain, who + ": every output is null", chunk_samples=-1, **outs)
