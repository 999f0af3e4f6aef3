"""Batched mirror of ``rosdyn::Chain`` (rosdyn_core/include/rosdyn_core/primitives.h:235-555) over the
C-ABI of librdyn_hip.so.  Method names and argument meaning are the reference's; every ``q/Dq/DDq`` is a
batch: a ``torch.float64`` CUDA tensor of shape (N, n_active) (sample-major) or (n_active, N) with
``layout="element"``.  Outputs are CUDA tensors that alias nothing (fresh allocations, or the caller's
``out=``).  The arithmetic happens in the HIP kernels; torch only owns the memory and the stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from .feedback import ModelFeedback
from ._lib import LAYOUT_ELEMENT_MAJOR, LAYOUT_SAMPLE_MAJOR, Batch, RegressorLayout, check, lib


def _torch():
    import torch
    return torch


class Chain(object):
    """rosdyn::createChain(urdf, base_frame, tool_frame, gravity)  (primitives.h:566)."""

    def __init__(self, urdf_xml, base_frame, tool_frame, gravity=(0.0, 0.0, 0.0), _handle=None):
        if _handle is not None:
            self._h = _handle
            return
        if "<robot" not in urdf_xml:
            with open(urdf_xml) as f:
                urdf_xml = f.read()
        h = C.c_void_p()
        g = (C.c_double * 3)(*[float(x) for x in gravity])
        check(lib().rdyn_chain_from_urdf(urdf_xml.encode(), base_frame.encode(), tool_frame.encode(), g, C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib._lib is not None:
            _lib._lib.rdyn_chain_destroy(h)
            self._h = None

    def clone(self):                                  # primitives.h:554
        h = C.c_void_p()
        check(lib().rdyn_chain_clone(self._h, C.byref(h)))
        return Chain(None, None, None, _handle=h)

    # ---- getters, primitives.h:364-447
    def getLinksNumber(self):
        return lib().rdyn_chain_links_number(self._h)

    def getJointsNumber(self):
        return lib().rdyn_chain_joints_number(self._h)

    def getActiveJointsNumber(self):
        return lib().rdyn_chain_active_joints_number(self._h)

    def getLinksName(self):
        return [lib().rdyn_chain_link_name(self._h, i).decode() for i in range(self.getLinksNumber())]

    def getJointsName(self):
        return [lib().rdyn_chain_joint_name(self._h, i).decode() for i in range(self.getJointsNumber())]

    def getMoveableJointNames(self):
        return [lib().rdyn_chain_moveable_joint_name(self._h, i).decode()
                for i in range(lib().rdyn_chain_moveable_joints_number(self._h))]

    def getActiveJointsName(self):
        return [lib().rdyn_chain_active_joint_name(self._h, i).decode() for i in range(self.getActiveJointsNumber())]

    def getJointTypes(self):
        return [lib().rdyn_chain_joint_type(self._h, i) for i in range(self.getJointsNumber())]

    def getGravity(self):
        g = (C.c_double * 3)()
        check(lib().rdyn_chain_gravity(self._h, g))
        return np.array(g[:])

    def setInputJointsName(self, names):              # primitives.h:362; returns bool like the reference
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        st = lib().rdyn_chain_set_input_joints(self._h, arr, len(names))
        if st == 6:
            return False
        check(st)
        return True

    def _limits(self, which):
        n = self.getActiveJointsNumber()
        bufs = [np.zeros(n) for _ in range(5)]
        check(lib().rdyn_chain_limits(self._h, *[b.ctypes.data_as(C.POINTER(C.c_double)) for b in bufs]))
        return bufs[which]

    def getQMax(self):
        return self._limits(0)

    def getQMin(self):
        return self._limits(1)

    def getDQMax(self):
        return self._limits(2)

    def getDDQMax(self):
        return self._limits(3)

    def getTauMax(self):
        return self._limits(4)

    def getNominalParameters(self):                   # primitives.h:548
        pi = np.zeros(10 * self.getJointsNumber())
        check(lib().rdyn_nominal_parameters(self._h, pi.ctypes.data_as(C.POINTER(C.c_double))))
        return pi

    def getBodyReduction(self):
        """Rigid-body reduction (include/rdyn.h: rdyn_chain_reduction; no reference counterpart): None when every chain joint is an
        input joint, else (body_joint (nJ,), X (nJ, 10, 10), pi_body (bodies, 10)) with
        Y[:, 10 f:10 f + 10] = Y[:, 10 b:10 b + 10] @ X[f], b = body_joint[f] (zero columns where b < 0)."""
        nj = self.getJointsNumber()
        body = np.zeros(nj, dtype=np.int32)
        X = np.zeros((nj, 10, 10))
        nb = lib().rdyn_chain_reduction(self._h, None, None, None)
        if nb <= 0:
            return None
        pi = np.zeros((nb, 10))
        lib().rdyn_chain_reduction(self._h, body.ctypes.data, X.ctypes.data, pi.ctypes.data)
        return body, X, pi

    # ---- batch plumbing
    def _batch(self, layout, q, dq=None, ddq=None):
        torch = _torch()
        n = self.getActiveJointsNumber()
        lay = LAYOUT_ELEMENT_MAJOR if layout == "element" else LAYOUT_SAMPLE_MAJOR
        ts = [t for t in (q, dq, ddq) if t is not None]
        for t in ts:
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
                raise ValueError("inputs must be contiguous 2-D float64 CUDA tensors")
            if t.shape != q.shape or t.device != q.device:
                raise ValueError("Input data dimensions mismatch")   # primitives_impl.h:1302
        N = q.shape[1] if lay == LAYOUT_ELEMENT_MAJOR else q.shape[0]
        nin = q.shape[0] if lay == LAYOUT_ELEMENT_MAJOR else q.shape[1]
        if nin != n:
            raise ValueError("Input data dimensions mismatch")
        b = Batch()
        b.n_samples = N
        b.q = q.data_ptr()
        b.dq = dq.data_ptr() if dq is not None else None
        b.ddq = ddq.data_ptr() if ddq is not None else None
        b.layout = lay
        b.device = q.device.index if q.device.index is not None else -1
        b.stream = torch.cuda.current_stream(q.device).cuda_stream
        return b, N, lay

    def _out(self, q, N, lay, rec_shape, out=None):
        torch = _torch()
        shape = (N,) + tuple(rec_shape) if lay == LAYOUT_SAMPLE_MAJOR else tuple(rec_shape) + (N,)
        if out is None:
            return torch.empty(shape, dtype=torch.float64, device=q.device)
        if tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous() or out.device != q.device:
            raise ValueError("out must be a contiguous float64 tensor of shape %s" % (shape,))
        return out

    def evaluateAll(self, q, Dq, DDq, layout="sample"):
        """include/rdyn.h: rdyn_evaluate_all -- every getter of the samples in ONE launch (chains of up to 10 joints; longer chains: the
        single-purpose launches).  Returns a dict with the records the single-purpose getters return: T_links, J, twists, dtwists, tau,
        tau_nonlinear, M, Y (per-sample Eigen images (N, P, n), or element-major (P, n, N))."""
        from ._lib import RegressorLayout
        b, N, lay = self._batch(layout, q, Dq, DDq)
        n, L, P = self.getActiveJointsNumber(), self.getLinksNumber(), 10 * self.getJointsNumber()
        o = dict(T_links=self._out(q, N, lay, (L, 4, 3)), J=self._out(q, N, lay, (n, 6)), twists=self._out(q, N, lay, (L, 6)),
                 dtwists=self._out(q, N, lay, (L, 6)), tau=self._out(q, N, lay, (n,)), tau_nonlinear=self._out(q, N, lay, (n,)),
                 M=self._out(q, N, lay, (n, n)), Y=self._out(q, N, lay, (P, n)))
        yl = RegressorLayout(n * P, 1, n) if lay == LAYOUT_SAMPLE_MAJOR else RegressorLayout(1, N, n * N)

        class _Out(C.Structure):
            _fields_ = [(k, C.c_void_p) for k in ("T_links", "J", "twists", "dtwists", "tau", "tau_nonlinear", "M", "Y", "y_layout")]
        rec = _Out(*([o[k].data_ptr() for k in ("T_links", "J", "twists", "dtwists", "tau", "tau_nonlinear", "M", "Y")] + [C.addressof(yl)]))
        check(lib().rdyn_evaluate_all(self._h, C.byref(b), C.byref(rec)))
        return o

    # ---- kinematics, primitives.h:452-463.  Record shapes are the transposes of the Eigen (column-major) objects:
    #      sample-major T[s] is (4, 3) = columns of the 3x4 [R | p]; use .transpose(-1, -2) for the matrix.
    def getTransformation(self, q, layout="sample", out=None):
        b, N, lay = self._batch(layout, q)
        T = self._out(q, N, lay, (4, 3), out)
        check(lib().rdyn_transformation(self._h, C.byref(b), T.data_ptr(), None))
        return T

    def getTransformations(self, q, layout="sample", out=None):
        b, N, lay = self._batch(layout, q)
        T = self._out(q, N, lay, (self.getLinksNumber(), 4, 3), out)
        check(lib().rdyn_transformation(self._h, C.byref(b), None, T.data_ptr()))
        return T

    def getJacobian(self, q, layout="sample", out=None):
        b, N, lay = self._batch(layout, q)
        J = self._out(q, N, lay, (self.getActiveJointsNumber(), 6), out)
        check(lib().rdyn_jacobian(self._h, C.byref(b), J.data_ptr()))
        return J

    def _link_index(self, link_name):
        names = self.getLinksName()
        if link_name not in names:
            raise ValueError("link " + link_name + " is not member of the chain")     # primitives_impl.h:920, 960, 1022
        return names.index(link_name)

    def getJacobianLink(self, q, link_name, layout="sample", out=None):              # primitives.h:456
        b, N, lay = self._batch(layout, q)
        J = self._out(q, N, lay, (self.getActiveJointsNumber(), 6), out)
        check(lib().rdyn_jacobian_link(self._h, C.byref(b), self._link_index(link_name), J.data_ptr()))
        return J

    def getTransformationLink(self, q, link_name, layout="sample"):                  # primitives.h:453
        T = self.getTransformations(q, layout=layout)
        i = self._link_index(link_name)
        return T[:, i] if layout != "element" else T[i]

    def getTwistLink(self, q, Dq, link_name, layout="sample"):                       # primitives.h:458
        tw = self.getTwist(q, Dq, layout=layout)
        i = self._link_index(link_name)
        return tw[:, i] if layout != "element" else tw[i]

    # ---- local inverse kinematics, primitives.h:510, 526 (batched: one pose per batch entry)
    def computeLocalIk(self, T_b_t, seed, toll=1e-4, max_iterations=100, weight=None, layout="sample", out=None, damping=0.0):
        """Returns (sol, status, iterations); status 1 = the reference's `true`, 0 = `false` (iteration cap instead of
        the reference's max_time), < 0 = the QP of that pose failed (see include/rdyn.h).  T_b_t: the record
        getTransformation returns ((N, 4, 3) sample-major / (4, 3, N) element-major)."""
        torch = _torch()
        b, N, lay = self._batch(layout, seed)
        shape = (N, 4, 3) if lay == LAYOUT_SAMPLE_MAJOR else (4, 3, N)
        if (tuple(T_b_t.shape) != shape or T_b_t.dtype != torch.float64 or not T_b_t.is_contiguous()
                or T_b_t.device != seed.device):
            raise ValueError("T_b_t must be a contiguous float64 tensor of shape %s" % (shape,))
        sol = self._out(seed, N, lay, (self.getActiveJointsNumber(),), out)
        status = torch.empty(N, dtype=torch.int32, device=seed.device)
        iters = torch.empty(N, dtype=torch.int32, device=seed.device)
        w = None
        if weight is not None:
            w = (C.c_double * 6)(*[float(v) for v in weight])
        # damping > 0: Levenberg term (no reference counterpart; what 7-DOF arms need, see include/rdyn.h)
        check(lib().rdyn_local_ik_damped(self._h, C.byref(b), T_b_t.data_ptr(), w, float(toll), float(damping), int(max_iterations),
                                         sol.data_ptr(), status.data_ptr(), iters.data_ptr()))
        return sol, status, iters

    def computeWeigthedLocalIk(self, T_b_t, weight, seed, toll=1e-4, max_iterations=100, layout="sample", out=None, damping=0.0):
        return self.computeLocalIk(T_b_t, seed, toll, max_iterations, weight=weight, layout=layout, out=out, damping=damping)

    def getMultiplicity(self, q):                                                    # primitives_impl.h:1470-1516
        """Host-side: every joint vector equal to q up to whole turns of the revolute input joints within the limits."""
        q = np.asarray(q, dtype=np.float64)
        qmax, qmin = self.getQMax(), self.getQMin()
        names, types = self.getJointsName(), self.getJointTypes()
        axes = []
        for idx, name in enumerate(self.getActiveJointsName()):
            vals = [q[idx]]
            if types[names.index(name)] == 0:   # REVOLUTE (continuous included, primitives_impl.h:74-77)
                if qmax[idx] - qmin[idx] > 2 * np.pi * 1e4:
                    # the reference enumerates every turn up to the 1e10 default limit; refuse instead of exhausting memory
                    raise ValueError("getMultiplicity: joint %s has no finite position limits" % name)
                tmp = q[idx]
                while True:
                    tmp += 2 * np.pi
                    if tmp > qmax[idx]:
                        break
                    vals.append(tmp)
                tmp = q[idx]
                while True:
                    tmp -= 2 * np.pi
                    if tmp < qmin[idx]:
                        break
                    vals.append(tmp)
            axes.append(vals)
        multiturn = [q.copy()]
        for idx, vals in enumerate(axes):
            size = len(multiturn)
            for v in vals[1:]:
                for im in range(size):
                    new_q = multiturn[im].copy()
                    new_q[idx] = v
                    multiturn.append(new_q)
        return multiturn

    def getTwist(self, q, Dq, layout="sample", out=None):
        b, N, lay = self._batch(layout, q, Dq)
        tw = self._out(q, N, lay, (self.getLinksNumber(), 6), out)
        check(lib().rdyn_twist(self._h, C.byref(b), tw.data_ptr(), None))
        return tw

    def getDTwist(self, q, Dq, DDq, layout="sample", out=None):
        b, N, lay = self._batch(layout, q, Dq, DDq)
        tw = self._out(q, N, lay, (self.getLinksNumber(), 6), out)
        check(lib().rdyn_twist(self._h, C.byref(b), None, tw.data_ptr()))
        return tw

    def _parts(self, q, Dq, DDq, DDDq, layout, which):
        b, N, lay = self._batch(layout, q, Dq, DDq)
        out = self._out(q, N, lay, (self.getLinksNumber(), 6))
        ptrs = [None, None, None]
        ptrs[which] = out.data_ptr()
        check(lib().rdyn_twist_parts(self._h, C.byref(b), DDDq.data_ptr() if DDDq is not None else None, *ptrs))
        return out

    def getDTwistLinearPart(self, q, DDq, layout="sample"):            # primitives.h:468
        return self._parts(q, None, DDq, None, layout, 0)

    def getDTwistNonLinearPart(self, q, Dq, layout="sample"):          # primitives.h:473
        return self._parts(q, Dq, None, None, layout, 1)

    def getDDTwist(self, q, Dq, DDq, DDDq, layout="sample"):           # primitives.h:488
        return self._parts(q, Dq, DDq, DDDq, layout, 2)

    def getDDTwistLinearPart(self, q, DDDq, layout="sample"):          # primitives.h:476
        b, N, lay = self._batch(layout, q)
        out = self._out(q, N, lay, (self.getLinksNumber(), 6))
        check(lib().rdyn_jerk_parts(self._h, C.byref(b), DDDq.data_ptr(), out.data_ptr(), None))
        return out

    def getDDTwistNonLinearPart(self, q, Dq, DDq, layout="sample"):    # primitives.h:480
        b, N, lay = self._batch(layout, q, Dq, DDq)
        out = self._out(q, N, lay, (self.getLinksNumber(), 6))
        check(lib().rdyn_jerk_parts(self._h, C.byref(b), None, None, out.data_ptr()))
        return out

    def getWrench(self, q, Dq, DDq, ext_wrenches_in_link_frame=None, layout="sample", out=None):      # primitives.h:530
        """Link wrenches (N, L, 6) / (L, 6, N), base-frame coordinates at the link origins; [:, -1] is getWrenchTool."""
        b, N, lay = self._batch(layout, q, Dq, DDq)
        w = self._out(q, N, lay, (self.getLinksNumber(), 6), out)
        ext = ext_wrenches_in_link_frame.data_ptr() if ext_wrenches_in_link_frame is not None else None
        check(lib().rdyn_wrench(self._h, C.byref(b), ext, w.data_ptr()))
        return w

    def jointIndex(self, name):                                         # primitives.h:447: -1 when not an input joint
        names = self.getActiveJointsName()
        return names.index(name) if name in names else -1

    def getJointTorqueExt(self, q, Dq, DDq, ext_wrenches_in_link_frame, layout="sample", out=None):   # primitives.h:539
        """ext: (N, L, 6) for layout="sample", (L, 6, N) for "element"."""
        b, N, lay = self._batch(layout, q, Dq, DDq)
        tau = self._out(q, N, lay, (self.getActiveJointsNumber(),), out)
        check(lib().rdyn_joint_torque_ext(self._h, C.byref(b), ext_wrenches_in_link_frame.data_ptr(), tau.data_ptr()))
        return tau

    # ---- dynamics, primitives.h:539-547
    def getJointTorque(self, q, Dq, DDq, layout="sample", out=None):
        b, N, lay = self._batch(layout, q, Dq, DDq)
        tau = self._out(q, N, lay, (self.getActiveJointsNumber(),), out)
        check(lib().rdyn_joint_torque(self._h, C.byref(b), tau.data_ptr()))
        return tau

    def getJointTorqueNonLinearPart(self, q, Dq, layout="sample", out=None):
        b, N, lay = self._batch(layout, q, Dq)
        tau = self._out(q, N, lay, (self.getActiveJointsNumber(),), out)
        check(lib().rdyn_joint_torque_nonlinear(self._h, C.byref(b), tau.data_ptr()))
        return tau

    def getJointInertia(self, q, layout="sample", out=None):
        b, N, lay = self._batch(layout, q)
        n = self.getActiveJointsNumber()
        M = self._out(q, N, lay, (n, n), out)
        check(lib().rdyn_joint_inertia(self._h, C.byref(b), M.data_ptr()))
        return M

    def _component_list(self, components):
        """(pointer, count) of a ComponentSet for the calls that take a component list"""
        assert components.n_active == self.getActiveJointsNumber(), "the ComponentSet was made for another number of active joints"
        return C.cast(components._arr, C.c_void_p), components.n_comps

    def _ext_wrenches(self, q, N, lay, ext_wrenches, ext_link, steps=None):
        """The rdyn_ext_wrenches of a call: one record is (N, links, 6) / (links * 6, N) for every link (ext_link None), (N, 6) / (6, N)
        for the link named ext_link.  steps None: one record; otherwise a leading dimension of at least `steps` records makes the
        sequence per step, without it the wrenches are constant over the horizon."""
        torch = _torch()
        w = ext_wrenches
        if w.dtype != torch.float64 or not w.is_cuda or not w.is_contiguous() or w.device != q.device:
            raise ValueError("inputs must be contiguous float64 CUDA tensors")
        L = self.getLinksNumber()
        if ext_link is None:
            rec, link = ((N, L, 6) if lay == LAYOUT_SAMPLE_MAJOR else (L * 6, N)), -1
        else:
            rec, link = ((N, 6) if lay == LAYOUT_SAMPLE_MAJOR else (6, N)), self._link_index(ext_link)
        x = _lib.ExtWrenches()
        x.w, x.link, x.step_stride = w.data_ptr(), link, 0
        if tuple(w.shape) == rec:
            return x
        if steps is not None and w.dim() == len(rec) + 1 and tuple(w.shape[1:]) == rec and w.shape[0] >= steps:
            x.step_stride = w[0].numel()
            return x
        raise ValueError("Input data dimensions mismatch")

    def _like_wrenches(self, shape_of, out, key):
        """an output shaped like the wrench tensor shape_of (or its shape): out when given and matching, otherwise new"""
        torch = _torch()
        shape = tuple(shape_of) if isinstance(shape_of, (tuple, list)) else tuple(shape_of.shape)
        if out is None:
            dev = shape_of.device if hasattr(shape_of, "device") else None
            return torch.empty(shape, dtype=torch.float64, device=dev)
        if tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out[%r] must be a contiguous float64 CUDA tensor of shape %s" % (key, shape))
        return out

    def getJointAcceleration(self, q, Dq, tau, layout="sample", out=None, chunk_samples=0, workspace=None, components=None,
                             ext_wrenches=None, ext_link=None):
        """Forward dynamics (include/rdyn.h: rdyn_forward_dynamics; no reference counterpart): DDq solves
        getJointInertia(q) DDq = tau - getJointTorqueNonLinearPart(q, Dq) per sample.  Returns (DDq, status): status (N,) int32, 1 solved,
        -1 the inertia matrix is not positive definite (that sample's DDq is NaN).  out may be tau itself.
        components: None, or a ComponentSet (friction, springs) whose torque at (q, Dq) is subtracted from tau first
        (rdyn_forward_dynamics_components).
        ext_wrenches: None, or external wrenches [force; torque] applied TO the links, in each link's own frame, as getJointTorqueExt
        takes them: (N, links, 6) for layout="sample", (links * 6, N) for "element"; with ext_link (a link name as in getJacobianLink)
        the wrench of that one link, (N, 6) / (6, N).  Their joint torque is subtracted inside the evaluation (rdyn_forward_dynamics_ext)."""
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, tau)
        b.ddq = None
        DDq = self._out(q, N, lay, (self.getActiveJointsNumber(),), out)
        status = torch.empty((N,), dtype=torch.int32, device=q.device)
        ext = self._ext_wrenches(q, N, lay, ext_wrenches, ext_link) if ext_wrenches is not None else None
        if ext is not None:
            nbytes = lib().rdyn_forward_dynamics_ext_workspace_bytes(self._h, C.byref(ext), chunk_samples)
        else:
            nbytes = lib().rdyn_forward_dynamics_workspace_bytes(self._h, chunk_samples)
        if workspace is None and nbytes > 0:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        ws = (workspace.data_ptr() if workspace is not None else None, workspace.numel() if workspace is not None else 0)
        if ext is not None:
            comps, n_comps = self._component_list(components) if components is not None else (None, 0)
            check(lib().rdyn_forward_dynamics_ext(self._h, C.byref(b), comps, n_comps, C.byref(ext), tau.data_ptr(), DDq.data_ptr(),
                                                  status.data_ptr(), chunk_samples, *ws))
        elif components is None:
            check(lib().rdyn_forward_dynamics(self._h, C.byref(b), tau.data_ptr(), DDq.data_ptr(), status.data_ptr(), chunk_samples, *ws))
        else:
            comps, n_comps = self._component_list(components)
            check(lib().rdyn_forward_dynamics_components(self._h, C.byref(b), comps, n_comps, tau.data_ptr(), DDq.data_ptr(),
                                                         status.data_ptr(), chunk_samples, *ws))
        return DDq, status

    def _feedback(self, q0, feedback, steps):
        """The rdyn_feedback of a closed-loop rollout from a rosdyn_amd.Feedback (shape rules there)"""
        torch = _torch()
        n, rec = self.getActiveJointsNumber(), tuple(q0.shape)

        def dev(t):
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.device != q0.device:
                raise ValueError("inputs must be contiguous float64 CUDA tensors")
            return t

        f = _lib.Feedback()
        strides = set()
        for name, ref in (("q_ref", feedback.q_ref), ("dq_ref", feedback.Dq_ref)):
            if ref is None:
                if name == "q_ref":
                    raise ValueError("feedback needs q_ref and kp")
                continue
            dev(ref)
            if tuple(ref.shape) == rec:
                strides.add(0)
            elif ref.dim() == len(rec) + 1 and tuple(ref.shape[1:]) == rec and ref.shape[0] >= steps:
                strides.add(q0.numel())
            else:
                raise ValueError("Input data dimensions mismatch")
            setattr(f, name, ref.data_ptr())
        if len(strides) != 1:
            raise ValueError("q_ref and Dq_ref must both be per step or both constant")
        f.ref_step_stride = strides.pop()
        if feedback.kp is None:
            raise ValueError("feedback needs q_ref and kp")
        shapes = set()
        for name, g in (("kp", feedback.kp), ("kd", feedback.kd)):
            if g is None:
                continue
            dev(g)
            if tuple(g.shape) not in ((n,), rec):
                raise ValueError("Input data dimensions mismatch")
            shapes.add(tuple(g.shape))
            setattr(f, name, g.data_ptr())
        if len(shapes) != 1:
            raise ValueError("kp and kd must both be shared or both per sample")
        f.gains_per_sample = 0 if shapes.pop() == (n,) else 1
        f.hold = 1 if feedback.hold else 0
        if feedback.tau_limit is not None:
            if tuple(dev(feedback.tau_limit).shape) != (n,):
                raise ValueError("Input data dimensions mismatch")
            f.tau_limit = feedback.tau_limit.data_ptr()
        return f

    def _model_feedback(self, q0, feedback, fb, steps):
        """The rdyn_model_feedback of a rosdyn_amd.ModelFeedback; fb: its rdyn_feedback (the acceleration reference shares its step stride)"""
        torch = _torch()
        if not isinstance(feedback.model, Chain):
            raise ValueError("ModelFeedback needs a Chain as its model")
        m = _lib.ModelFeedback()
        m.model, m.law = feedback.model._h, _lib.LAWS[feedback.law]
        ref = feedback.DDq_ref
        if ref is not None:
            if ref.dtype != torch.float64 or not ref.is_cuda or not ref.is_contiguous() or ref.device != q0.device:
                raise ValueError("inputs must be contiguous float64 CUDA tensors")
            rec = tuple(q0.shape)
            per_step = ref.dim() == len(rec) + 1 and tuple(ref.shape[1:]) == rec and ref.shape[0] >= steps
            if not (tuple(ref.shape) == rec or per_step):
                raise ValueError("Input data dimensions mismatch")
            if (q0.numel() if per_step else 0) != fb.ref_step_stride:
                raise ValueError("q_ref and DDq_ref must both be per step or both constant")
            m.ddq_ref = ref.data_ptr()
        return m

    def rollout(self, q0, Dq0, tau, dt, integrator="rk4", n_steps=None, layout="sample", trajectory_every=0, out=None, chunk_samples=0,
                workspace=None, components=None, ext_wrenches=None, ext_link=None, feedback=None):
        """Rollout (include/rdyn.h: rdyn_rollout; no reference counterpart): n_steps integrator steps of size dt of the forward dynamics
        from (q0, Dq0), the torques held over each step.  integrator: "rk4" or "semi_implicit_euler" ("euler").
        tau: (T, N, n) for layout="sample", (T, n, N) for "element" -- n_steps defaults to T and may be smaller; or (N, n) / (n, N) with an
        explicit n_steps: the same torques at every step.
        Returns (q_end, Dq_end, status), and with trajectory_every = k >= 1 also (q_traj, Dq_traj): n_steps // k records, record r = the
        state after step (r + 1) k, shaped (records,) + q0.shape.  status (N,) int32: 1, or -1 from the step on at which the inertia
        matrix was not positive definite (NaN state from then on).  out: None or (q_end, Dq_end) tensors; they may be q0 and Dq0.
        components: None, or a ComponentSet (friction, springs) whose torque is subtracted from tau at every integrator stage, at the
        stage's own state (rdyn_rollout_components).
        ext_wrenches, ext_link: None, or external link wrenches as in getJointAcceleration, evaluated at every integrator stage at the
        stage's own q (rdyn_rollout_ext): one record -- (N, links, 6) / (links * 6, N), or (N, 6) / (6, N) with ext_link -- is constant
        over the horizon; a leading dimension T makes the sequence per step, held over each step like the torques.
        feedback: None, or a rosdyn_amd.Feedback: the closed loop (rdyn_rollout_feedback), tau its feed-forward term.  With
        feedback.command_trajectory and trajectory_every >= 1 the command trajectory is appended as the last returned tensor.  A
        rosdyn_amd.ModelFeedback runs a model-based law (computed torque, gravity compensation: rdyn_rollout_model_feedback), for the
        chains a Feedback runs in one launch; nothing more is allocated than for a Feedback."""
        torch = _torch()
        b, N, lay = self._batch(layout, q0, Dq0)
        if integrator not in _lib.INTEGRATORS:
            raise ValueError("unknown integrator %r" % (integrator,))
        if tau.dtype != torch.float64 or not tau.is_cuda or not tau.is_contiguous() or tau.device != q0.device:
            raise ValueError("inputs must be contiguous float64 CUDA tensors")
        if tau.dim() == 3 and tuple(tau.shape[1:]) == tuple(q0.shape):
            stride = q0.numel()
            if n_steps is None:
                n_steps = tau.shape[0]
            elif n_steps > tau.shape[0]:
                raise ValueError("Input data dimensions mismatch")
        elif tau.dim() == 2 and tuple(tau.shape) == tuple(q0.shape) and n_steps is not None:
            stride = 0
        else:
            raise ValueError("Input data dimensions mismatch")
        n = self.getActiveJointsNumber()
        q_end, dq_end = out if out is not None else (None, None)
        q_end, dq_end = self._out(q0, N, lay, (n,), q_end), self._out(q0, N, lay, (n,), dq_end)
        status = torch.empty((N,), dtype=torch.int32, device=q0.device)
        d = _lib.RolloutDesc()
        d.n_steps, d.integrator, d.dt = int(n_steps), _lib.INTEGRATORS[integrator], float(dt)
        d.tau, d.tau_step_stride = tau.data_ptr(), stride
        d.q_end, d.dq_end, d.status = q_end.data_ptr(), dq_end.data_ptr(), status.data_ptr()
        q_traj = dq_traj = None
        if trajectory_every:
            records = max(int(n_steps), 0) // int(trajectory_every) if trajectory_every > 0 else 0
            q_traj = torch.empty((records,) + tuple(q0.shape), dtype=torch.float64, device=q0.device)
            dq_traj = torch.empty_like(q_traj)
            d.q_traj, d.dq_traj = q_traj.data_ptr(), dq_traj.data_ptr()
            d.traj_step_stride, d.traj_every = q0.numel(), int(trajectory_every)
        ext = self._ext_wrenches(q0, N, lay, ext_wrenches, ext_link, steps=int(n_steps)) if ext_wrenches is not None else None
        fb = tau_traj = None
        mfb = None
        if feedback is not None:
            fb = self._feedback(q0, feedback, int(n_steps))
            if feedback.command_trajectory and trajectory_every:
                tau_traj = torch.empty_like(q_traj)
                fb.tau_traj = tau_traj.data_ptr()
            ext_p = C.byref(ext) if ext is not None else None
            if isinstance(feedback, ModelFeedback):
                mfb = self._model_feedback(q0, feedback, fb, int(n_steps))
                nbytes = lib().rdyn_rollout_model_feedback_workspace_bytes(self._h, C.byref(d), ext_p, C.byref(fb), C.byref(mfb), N, chunk_samples)
            else:
                nbytes = lib().rdyn_rollout_feedback_workspace_bytes(self._h, C.byref(d), ext_p, C.byref(fb), N, chunk_samples)
        elif ext is not None:
            nbytes = lib().rdyn_rollout_ext_workspace_bytes(self._h, C.byref(d), C.byref(ext), N, chunk_samples)
        else:
            nbytes = lib().rdyn_rollout_workspace_bytes(self._h, C.byref(d), N, chunk_samples)
        if workspace is None and nbytes > 0:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q0.device)
        ws = (workspace.data_ptr() if workspace is not None else None, workspace.numel() if workspace is not None else 0)
        if mfb is not None:
            comps, n_comps = self._component_list(components) if components is not None else (None, 0)
            check(lib().rdyn_rollout_model_feedback(self._h, C.byref(b), C.byref(d), comps, n_comps, ext_p, C.byref(fb), C.byref(mfb),
                                                    chunk_samples, *ws))
        elif fb is not None:
            comps, n_comps = self._component_list(components) if components is not None else (None, 0)
            check(lib().rdyn_rollout_feedback(self._h, C.byref(b), C.byref(d), comps, n_comps, ext_p, C.byref(fb), chunk_samples, *ws))
        elif ext is not None:
            comps, n_comps = self._component_list(components) if components is not None else (None, 0)
            check(lib().rdyn_rollout_ext(self._h, C.byref(b), C.byref(d), comps, n_comps, C.byref(ext), chunk_samples, *ws))
        elif components is None:
            check(lib().rdyn_rollout(self._h, C.byref(b), C.byref(d), chunk_samples, *ws))
        else:
            comps, n_comps = self._component_list(components)
            check(lib().rdyn_rollout_components(self._h, C.byref(b), C.byref(d), comps, n_comps, chunk_samples, *ws))
        if tau_traj is not None:
            return q_end, dq_end, status, q_traj, dq_traj, tau_traj
        if trajectory_every:
            return q_end, dq_end, status, q_traj, dq_traj
        return q_end, dq_end, status

    def getJointTorqueDerivatives(self, q, Dq, DDq, layout="sample", want=("dq", "dv"), out=None):
        """Derivatives of getJointTorque (include/rdyn.h: rdyn_joint_torque_derivatives; no reference counterpart).  want: any non-empty
        selection of "dq" (d tau / d q), "dv" (d tau / d Dq) and "M" (d tau / d DDq = getJointInertia); returns the tensors in the order of
        `want` (a single tensor when one name is given as a string).  Records as getJointInertia's: (N, n, n) with t[s, k, i] = d tau_i / d x_k
        (the transpose of the column-major n x n matrix) for layout="sample", (n, n, N) with t[k, i, s] for "element".
        out: None, or a dict name -> preallocated tensor."""
        single = isinstance(want, str)
        names = (want,) if single else tuple(want)
        if not names or len(set(names)) != len(names) or any(k not in ("dq", "dv", "M") for k in names):
            raise ValueError('want must be a non-empty selection of "dq", "dv", "M"')
        b, N, lay = self._batch(layout, q, Dq, DDq)
        n = self.getActiveJointsNumber()
        res = {k: self._out(q, N, lay, (n, n), (out or {}).get(k)) for k in names}
        ptr = [res[k].data_ptr() if k in res else None for k in ("dq", "dv", "M")]
        check(lib().rdyn_joint_torque_derivatives(self._h, C.byref(b), *ptr))
        return res[names[0]] if single else tuple(res[k] for k in names)

    def getJointAccelerationDerivatives(self, q, Dq, tau, layout="sample", want=("dq", "dv", "dtau"), out=None, components=None,
                                        chunk_samples=0, workspace=None):
        """Derivatives of getJointAcceleration (include/rdyn.h: rdyn_forward_dynamics_derivatives; no reference counterpart).  want: any
        non-empty selection of "dq" (d DDq / d q), "dv" (d DDq / d Dq) and "dtau" (d DDq / d tau = the inverse of getJointInertia); returns
        (DDq, status, *wanted) with the matrices in the order of `want` (a single name may be given as a string).  DDq and status are
        getJointAcceleration's (components included); a sample with status -1 is NaN everywhere.  Records as getJointTorqueDerivatives':
        (N, n, n) with t[s, k, i] = d DDq_i / d x_k for layout="sample", (n, n, N) with t[k, i, s] for "element".
        out: None, or a dict name -> preallocated tensor; the key "ddq" names DDq, which may be tau itself."""
        single = isinstance(want, str)
        names = (want,) if single else tuple(want)
        if not names or len(set(names)) != len(names) or any(k not in ("dq", "dv", "dtau") for k in names):
            raise ValueError('want must be a non-empty selection of "dq", "dv", "dtau"')
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, tau)
        b.ddq = None
        n = self.getActiveJointsNumber()
        DDq = self._out(q, N, lay, (n,), (out or {}).get("ddq"))
        res = {k: self._out(q, N, lay, (n, n), (out or {}).get(k)) for k in names}
        ptr = [res[k].data_ptr() if k in res else None for k in ("dq", "dv", "dtau")]
        status = torch.empty((N,), dtype=torch.int32, device=q.device)
        nbytes = lib().rdyn_forward_dynamics_derivatives_workspace_bytes(self._h, chunk_samples)
        if workspace is None and nbytes > 0:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        ws = (workspace.data_ptr() if workspace is not None else None, workspace.numel() if workspace is not None else 0)
        comps, n_comps = self._component_list(components) if components is not None else (None, 0)
        check(lib().rdyn_forward_dynamics_derivatives(self._h, C.byref(b), comps, n_comps, tau.data_ptr(), DDq.data_ptr(), *ptr,
                                                      status.data_ptr(), chunk_samples, *ws))
        return (DDq, status) + tuple(res[k] for k in names)

    def getJointAccelerationVjp(self, q, Dq, tau, DDq_bar, layout="sample", want=("q", "dq", "tau"), components=None, out=None,
                                chunk_samples=0, workspace=None, ext_wrenches=None, ext_link=None):
        """Reverse-mode product of getJointAcceleration (include/rdyn.h: rdyn_forward_dynamics_vjp; no reference counterpart): for the seed
        DDq_bar on DDq, "q" -> (d DDq / d q)' DDq_bar, "dq" -> (d DDq / d Dq)' DDq_bar, "tau" -> M^-1 DDq_bar, the matrices those of
        getJointAccelerationDerivatives (components and their slopes included) -- never formed.  want: a selection with at least one of the
        three; "ddq" may be added and names DDq itself (getJointAcceleration's bits).  Returns (status, *wanted) in the order of `want` (a
        single name may be given as a string); every vector is shaped like q.  status (N,) int32: 1, or -1 (the inertia matrix is not
        positive definite, or q, Dq, tau or DDq_bar of the sample is not finite): that sample is NaN in every output.
        out: None, or a dict name -> preallocated tensor; out["tau"] may be DDq_bar itself.
        ext_wrenches, ext_link: None, or external link wrenches as in getJointAcceleration (rdyn_forward_dynamics_vjp_ext): the product
        is that of getJointAcceleration(ext_wrenches=), "q" gains the dependence of the wrench torque on q, and want may name "ext":
        the gradient with respect to the wrenches, shaped like ext_wrenches (the base link's record 0); a non-finite wrench entry the
        sample reads gives status -1."""
        single = isinstance(want, str)
        names = (want,) if single else tuple(want)
        allowed = ("q", "dq", "tau", "ddq") + (("ext",) if ext_wrenches is not None else ())
        if (not names or len(set(names)) != len(names) or any(k not in allowed for k in names)
                or not any(k != "ddq" for k in names)):
            raise ValueError('want must be a selection of "q", "dq", "tau" (at least one) and "ddq"'
                             if ext_wrenches is None else 'want must be a selection of "q", "dq", "tau", "ext" (at least one) and "ddq"')
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, tau)
        b.ddq = None
        if (DDq_bar.shape != q.shape or DDq_bar.dtype != torch.float64 or not DDq_bar.is_cuda or not DDq_bar.is_contiguous()
                or DDq_bar.device != q.device):
            raise ValueError("Input data dimensions mismatch")
        n = self.getActiveJointsNumber()
        res = {k: self._out(q, N, lay, (n,), (out or {}).get(k)) for k in names if k != "ext"}
        ptr = [res[k].data_ptr() if k in res else None for k in ("q", "dq", "tau", "ddq")]
        status = torch.empty((N,), dtype=torch.int32, device=q.device)
        if ext_wrenches is not None:
            ext = self._ext_wrenches(q, N, lay, ext_wrenches, ext_link)
            if "ext" in names:
                res["ext"] = self._like_wrenches(ext_wrenches, (out or {}).get("ext"), "ext")
            comps, n_comps = self._component_list(components) if components is not None else (None, 0)
            check(lib().rdyn_forward_dynamics_vjp_ext(self._h, C.byref(b), comps, n_comps, C.byref(ext), tau.data_ptr(), DDq_bar.data_ptr(),
                                                      ptr[0], ptr[1], ptr[2], res["ext"].data_ptr() if "ext" in res else None, ptr[3],
                                                      status.data_ptr(), chunk_samples, None, 0))
            return (status,) + tuple(res[k] for k in names)
        nbytes = lib().rdyn_forward_dynamics_vjp_workspace_bytes(self._h, chunk_samples)
        if workspace is None and nbytes > 0:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        ws = (workspace.data_ptr() if workspace is not None else None, workspace.numel() if workspace is not None else 0)
        comps, n_comps = self._component_list(components) if components is not None else (None, 0)
        check(lib().rdyn_forward_dynamics_vjp(self._h, C.byref(b), comps, n_comps, tau.data_ptr(), DDq_bar.data_ptr(), *ptr,
                                              status.data_ptr(), chunk_samples, *ws))
        return (status,) + tuple(res[k] for k in names)

    def getJointAccelerationParameterVjp(self, q, Dq, tau, DDq_bar, components=None, layout="sample", reduce=False, accumulate=None,
                                         chunk_samples=0, workspace=None):
        """Reverse-mode product of getJointAcceleration with respect to the model's PARAMETERS (include/rdyn.h:
        rdyn_forward_dynamics_parameter_vjp; no reference counterpart): with w = M^-1 DDq_bar,
        pi_bar = -getRegressor(q, Dq, DDq)' w (P = 10 getJointsNumber() entries, the order of getNominalParameters) and
        comp_bar = -(component regressor)' w (components.columns entries), DDq = getJointAcceleration's.  Neither regressor is formed.
        Returns (pi_bar, comp_bar, tau_bar, DDq, status).  reduce=False: the per-sample rows, (N, P) and (N, K) for layout="sample",
        (P, N) and (K, N) for "element"; a status -1 sample is NaN in its rows.  reduce=True: the sums (P,) and (K,) over the samples
        with status 1, reproducible bit for bit from run to run; accumulate = (pi_sum, comp_sum) adds to those tensors instead
        (comp_sum may be None without components).  comp_bar is None without components.  tau_bar and DDq are those of
        getJointAccelerationVjp.  chunk_samples, workspace: as in getJointAccelerationVjp (more than 10 input joints run in chunks; the
        results do not depend on the chunk size)."""
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, tau)
        b.ddq = None
        if (DDq_bar.shape != q.shape or DDq_bar.dtype != torch.float64 or not DDq_bar.is_cuda or not DDq_bar.is_contiguous()
                or DDq_bar.device != q.device):
            raise ValueError("Input data dimensions mismatch")
        n, P = self.getActiveJointsNumber(), 10 * self.getJointsNumber()
        comps, n_comps = self._component_list(components) if components is not None else (None, 0)
        K = components.columns if components is not None else 0
        tau_bar, DDq = self._out(q, N, lay, (n,)), self._out(q, N, lay, (n,))
        status = torch.empty((N,), dtype=torch.int32, device=q.device)
        rows = [None, None]
        sums = [None, None]
        acc = 0
        if reduce:
            if accumulate is not None:
                sums, acc = list(accumulate), 1
                for t, size in zip(sums, (P, K)):
                    if t is not None and (tuple(t.shape) != (size,) or t.dtype != torch.float64 or not t.is_contiguous()
                                          or t.device != q.device):
                        raise ValueError("accumulate must hold contiguous float64 tensors of %d and %d entries" % (P, K))
            else:
                sums = [torch.empty((P,), dtype=torch.float64, device=q.device),
                        torch.empty((K,), dtype=torch.float64, device=q.device) if K else None]
        else:
            rows = [self._out(q, N, lay, (P,)), self._out(q, N, lay, (K,)) if K else None]
        nbytes = lib().rdyn_forward_dynamics_parameter_vjp_workspace_bytes(self._h, comps, n_comps, N, chunk_samples)
        if workspace is None and nbytes > 0:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        ws = (workspace.data_ptr() if workspace is not None else None, workspace.numel() if workspace is not None else 0)
        ptr = [t.data_ptr() if t is not None else None for t in rows + sums]
        check(lib().rdyn_forward_dynamics_parameter_vjp(self._h, C.byref(b), comps, n_comps, tau.data_ptr(), DDq_bar.data_ptr(), *ptr, acc,
                                                        tau_bar.data_ptr(), DDq.data_ptr(), status.data_ptr(), chunk_samples, *ws))
        res = sums if reduce else rows
        return res[0], res[1], tau_bar, DDq, status

    def withParameters(self, pi):
        """The chain with the inertial parameters pi (include/rdyn.h: rdyn_chain_with_parameters; no reference counterpart): a new,
        independent Chain equal to clone() in everything else, input-joint selection included.  pi: 10 getJointsNumber() values in the
        order of getNominalParameters (host numpy array or CPU tensor); they are stored as given, so getNominalParameters of the
        result returns them bit for bit.  Values that are not finite raise ValueError."""
        pi = np.ascontiguousarray(np.asarray(pi, dtype=np.float64).reshape(-1))
        if pi.size != 10 * self.getJointsNumber():
            raise ValueError("pi must hold 10 values per chain joint (%d)" % (10 * self.getJointsNumber(),))
        h = C.c_void_p()
        check(lib().rdyn_chain_with_parameters(self._h, pi.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)))
        return Chain(None, None, None, _handle=h)

    def rolloutAdjoint(self, q0, Dq0, tau, dt, q_traj, Dq_traj, gq_end=None, gDq_end=None, gq_traj=None, gDq_traj=None, integrator="rk4",
                       n_steps=None, layout="sample", components=None, sum_tau=False, out=None, chunk_samples=0, workspace=None,
                       ext_wrenches=None, ext_link=None, want_ext=False, sum_ext=False, feedback=None, want_feedback=(), gu_traj=None,
                       accumulate=False, sum_ref=None):
        """Adjoint of rollout (include/rdyn.h: rdyn_rollout_adjoint; no reference counterpart): the exact transpose of the n_steps
        integrator steps rollout takes, from the seeds on the end state (gq_end, gDq_end, shaped like q0; None = 0) and, optionally, on
        every trajectory record (gq_traj, gDq_traj: (>= n_steps,) + q0.shape, record k seeds the state after step k + 1) back to the
        gradients with respect to (q0, Dq0) and the torques.  q0, Dq0, tau, dt, integrator, n_steps, layout, components: the forward
        call's, with rollout's shape rules.  q_traj, Dq_traj: that call's trajectory with trajectory_every=1 ((>= n_steps - 1,) + q0.shape;
        None is allowed for n_steps <= 1).
        Returns (gq0, gDq0, gtau, status).  gtau: (n_steps,) + q0.shape, one gradient per step, or shaped like q0 with sum_tau=True (the
        sum over the steps: the gradient of torques held over the whole horizon).  status (N,) int32: 1, or -1 when an evaluation of the
        sample failed or met a non-finite value -- a sample whose forward rollout reported -1 in particular: NaN in every gradient.
        out: None, or a dict with any of "gq0", "gDq0", "gtau" -> preallocated tensor; out["gq0"] / out["gDq0"] may be gq_end / gDq_end.
        ext_wrenches, ext_link: the forward call's external link wrenches, with rollout's shape rules (rdyn_rollout_adjoint_ext): the
        transpose is that of rollout(ext_wrenches=).  want_ext=True appends gext to the returned tuple, the gradient with respect to the
        wrenches: (n_steps,) + one record's shape, one gradient per step, or one record with sum_ext=True (the sum over the steps: the
        gradient of a wrench held over the horizon); out may hold "gext".
        feedback: the forward call's rosdyn_amd.Feedback (rdyn_rollout_adjoint_feedback): the transpose is that of rollout(feedback=), the
        PD law and its clamp included, and gtau is the gradient with respect to the feed-forward torques.  want_feedback: any selection
        of "q_ref", "Dq_ref", "kp", "kd", "tau_limit"; their gradients are appended to the returned tuple in that order (behind gext):
          q_ref, Dq_ref     (n_steps,) + q0.shape, one gradient per step, where the reference is per step; shaped like q0, the sum over
                            the steps, where it is a constant set point.  sum_ref=True / False overrides the choice.
          kp, kd, tau_limit shaped like q0: one row per SAMPLE summed over the steps, also for shared gains and the shared limits -- sum the
                            rows over the samples for their gradient.
        out may hold them as "gq_ref", "gDq_ref", "gkp", "gkd", "gtau_limit"; accumulate=True continues adding to the sums that out holds
        (a horizon split into chained calls, the later part first).  gu_traj: None, or seeds on the command trajectory of
        rollout(feedback=Feedback(command_trajectory=True), trajectory_every=1): (>= n_steps,) + q0.shape.  Chains for which
        rollout(feedback=) takes its chunked route raise RdynError (RDYN_ERR_UNSUPPORTED)."""
        closed = None
        if feedback is not None:
            closed = (feedback, tuple(want_feedback), gu_traj, bool(accumulate), sum_ref)
        elif want_feedback or gu_traj is not None or accumulate or sum_ref is not None:
            raise ValueError("want_feedback, gu_traj, accumulate and sum_ref need feedback")
        if ext_wrenches is None:
            if want_ext or sum_ext or ext_link is not None:
                raise ValueError("want_ext, sum_ext and ext_link need ext_wrenches")
            return self._rollout_adjoint(q0, Dq0, tau, dt, q_traj, Dq_traj, gq_end, gDq_end, gq_traj, gDq_traj, integrator, n_steps, layout,
                                         components, sum_tau, out, chunk_samples, workspace, None, None, closed)
        return self._rollout_adjoint(q0, Dq0, tau, dt, q_traj, Dq_traj, gq_end, gDq_end, gq_traj, gDq_traj, integrator, n_steps, layout, components,
                                     sum_tau, out, chunk_samples, workspace, None, (ext_wrenches, ext_link, bool(want_ext), bool(sum_ext)), closed)

    def rolloutParameterAdjoint(self, q0, Dq0, tau, dt, q_traj, Dq_traj, gq_end=None, gDq_end=None, gq_traj=None, gDq_traj=None,
                                integrator="rk4", n_steps=None, layout="sample", components=None, sum_tau=False, out=None, chunk_samples=0,
                                workspace=None, accumulate=False, feedback=None, want_feedback=(), gu_traj=None, sum_ref=None,
                                ext_wrenches=None, ext_link=None):
        """rolloutAdjoint with the gradients with respect to the model's parameters (include/rdyn.h: rdyn_rollout_adjoint_parameters; no
        reference counterpart).  The arguments are rolloutAdjoint's; returns (gq0, gDq0, gtau, gpi, gcomp, status): the first three and the
        status are rolloutAdjoint's, bit for bit; gpi (10 getJointsNumber(),) = dL/d(inertial parameters, the order of
        getNominalParameters) and gcomp (components.columns,) = dL/d(component parameters, column order; None without components), each
        summed over the samples whose status is 1 -- a failed sample contributes nothing -- and reproducible bit for bit from run to run.
        out may also hold "gpi" and "gcomp": preallocated tensors, which accumulate=True adds to instead of overwriting (a horizon split into
        chained calls).  Chains with more than 10 input joints raise RdynError (RDYN_ERR_UNSUPPORTED).
        feedback: the forward call's rosdyn_amd.Feedback (rdyn_rollout_adjoint_feedback_parameters): the adjoint is that of
        rollout(feedback=) -- rolloutAdjoint(feedback=)'s bits in gq0, gDq0, gtau, the status and the law's gradients -- and gpi / gcomp are
        the parameter gradients of the closed loop, every product taken at the command the forward call applied.  want_feedback,
        gu_traj, sum_ref: as in rolloutAdjoint; returns (gq0, gDq0, gtau, gpi, gcomp, status) followed by the law's gradients in
        want_feedback order.  accumulate=True then continues the law's sums in out as well as gpi / gcomp (a split horizon wants both).
        ext_wrenches (with ext_link): the parameter gradients with external wrenches are not served yet; the library's
        RDYN_ERR_UNSUPPORTED is raised as RdynError."""
        closed = None
        if feedback is not None:
            closed = (feedback, tuple(want_feedback), gu_traj, bool(accumulate), sum_ref)
        elif want_feedback or gu_traj is not None or sum_ref is not None:
            raise ValueError("want_feedback, gu_traj and sum_ref need feedback")
        if ext_wrenches is None and ext_link is not None:
            raise ValueError("ext_link needs ext_wrenches")
        wrenches = None if ext_wrenches is None else (ext_wrenches, ext_link, False, False)
        return self._rollout_adjoint(q0, Dq0, tau, dt, q_traj, Dq_traj, gq_end, gDq_end, gq_traj, gDq_traj, integrator, n_steps, layout, components,
                                     sum_tau, out, chunk_samples, workspace, bool(accumulate), wrenches, closed)

    def _rollout_adjoint(self, q0, Dq0, tau, dt, q_traj, Dq_traj, gq_end, gDq_end, gq_traj, gDq_traj, integrator, n_steps, layout, components,
                         sum_tau, out, chunk_samples, workspace, accumulate, wrenches=None, closed=None):
        """the two calls above; accumulate None: without the parameter gradients; wrenches: None, or rolloutAdjoint's (ext_wrenches,
        ext_link, want_ext, sum_ext); closed: None, or rolloutAdjoint's (feedback, want_feedback, gu_traj, accumulate, sum_ref).  With
        the parameter gradients AND wrenches or a law: rdyn_rollout_adjoint_feedback_parameters"""
        if closed is not None and isinstance(closed[0], ModelFeedback):
            raise NotImplementedError("the adjoint of a model-based law (rosdyn_amd.ModelFeedback) is not served yet: rdyn_rollout_adjoint_feedback "
                                      "is the transpose of the PD law alone")
        torch = _torch()
        b, N, lay = self._batch(layout, q0, Dq0)
        if integrator not in _lib.INTEGRATORS:
            raise ValueError("unknown integrator %r" % (integrator,))

        def ok(t, lead=None):
            return (t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.device == q0.device
                    and (tuple(t.shape) == tuple(q0.shape) if lead is None
                         else t.dim() == 3 and tuple(t.shape[1:]) == tuple(q0.shape) and t.shape[0] >= lead))

        if tau.dim() == 3 and ok(tau, 0):
            stride = q0.numel()
            if n_steps is None:
                n_steps = tau.shape[0]
            elif n_steps > tau.shape[0]:
                raise ValueError("Input data dimensions mismatch")
        elif tau.dim() == 2 and ok(tau) and n_steps is not None:
            stride = 0
        else:
            raise ValueError("Input data dimensions mismatch")
        T = int(n_steps)
        if T >= 2 and (q_traj is None or Dq_traj is None):
            raise ValueError("two or more steps need the forward call's trajectory (trajectory_every=1)")
        for t, lead in ((q_traj, T - 1), (Dq_traj, T - 1), (gq_traj, T), (gDq_traj, T)):
            if t is not None and not ok(t, max(lead, 0)):
                raise ValueError("Input data dimensions mismatch")
        for t in (gq_end, gDq_end):
            if t is not None and not ok(t):
                raise ValueError("Input data dimensions mismatch")
        n = self.getActiveJointsNumber()
        out = out or {}
        gq0, gdq0 = self._out(q0, N, lay, (n,), out.get("gq0")), self._out(q0, N, lay, (n,), out.get("gDq0"))
        gshape = tuple(q0.shape) if sum_tau else (max(T, 0),) + tuple(q0.shape)
        gtau = out.get("gtau")
        if gtau is None:
            gtau = torch.empty(gshape, dtype=torch.float64, device=q0.device)
        elif tuple(gtau.shape) != gshape or gtau.dtype != torch.float64 or not gtau.is_contiguous() or gtau.device != q0.device:
            raise ValueError("out['gtau'] must be a contiguous float64 tensor of shape %s" % (gshape,))
        status = torch.empty((N,), dtype=torch.int32, device=q0.device)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() > 0 else None
        d = _lib.RolloutAdjointDesc()
        d.n_steps, d.integrator, d.dt = T, _lib.INTEGRATORS[integrator], float(dt)
        d.tau, d.tau_step_stride = tau.data_ptr(), stride
        d.q_traj, d.dq_traj, d.traj_step_stride = ptr(q_traj), ptr(Dq_traj), q0.numel()
        d.gq_end, d.gdq_end = ptr(gq_end), ptr(gDq_end)
        d.gq_traj, d.gdq_traj, d.gtraj_step_stride = ptr(gq_traj), ptr(gDq_traj), q0.numel()
        d.gq0, d.gdq0 = gq0.data_ptr(), gdq0.data_ptr()
        d.gtau, d.gtau_step_stride = ptr(gtau), 0 if sum_tau else q0.numel()
        d.status = status.data_ptr()
        comps, n_comps = self._component_list(components) if components is not None else (None, 0)
        if wrenches is not None or closed is not None:
            # rdyn_rollout_adjoint_feedback: without a law it is rdyn_rollout_adjoint_ext
            ext, g, gext, want_ext = None, _lib.ExtWrenchGradient(), None, False
            if wrenches is not None:
                ext_wrenches, ext_link, want_ext, sum_ext = wrenches
                ext = self._ext_wrenches(q0, N, lay, ext_wrenches, ext_link, steps=T)
                if want_ext:
                    rec = tuple(ext_wrenches.shape[1:]) if ext.step_stride else tuple(ext_wrenches.shape)
                    shape = rec if sum_ext else (max(T, 0),) + rec
                    gext = self._like_wrenches(shape, out.get("gext"), "gext") if out.get("gext") is not None else torch.empty(
                        shape, dtype=torch.float64, device=q0.device)
                    g.gw, g.step_stride = ptr(gext), 0 if sum_ext else int(torch.Size(rec).numel())
            fb, gf, grads = None, None, []
            if closed is not None:
                feedback, want_fb, gu_traj, fb_acc, sum_ref = closed
                fb = self._feedback(q0, feedback, T)
                gf = _lib.FeedbackGradient()
                gf.accumulate = 1 if fb_acc else 0
                if gu_traj is not None:
                    if not ok(gu_traj, max(T, 0)):
                        raise ValueError("Input data dimensions mismatch")
                    gf.gu_traj, gf.gu_step_stride = ptr(gu_traj), q0.numel()
                if sum_ref is None:
                    sum_ref = fb.ref_step_stride == 0
                fields = {"q_ref": ("gq_ref", "gq_ref"), "Dq_ref": ("gDq_ref", "gdq_ref"), "kp": ("gkp", "gkp"), "kd": ("gkd", "gkd"),
                          "tau_limit": ("gtau_limit", "glim")}
                for name in want_fb:
                    if name not in fields:
                        raise ValueError("want_feedback: unknown name %r" % (name,))
                    key, field = fields[name]
                    summed = sum_ref or name in ("kp", "kd", "tau_limit")
                    shape = tuple(q0.shape) if summed else (max(T, 0),) + tuple(q0.shape)
                    t = out.get(key)
                    if t is None:
                        if fb_acc and summed:
                            raise ValueError("accumulate=True needs out[%r]" % (key,))
                        t = torch.empty(shape, dtype=torch.float64, device=q0.device)
                    elif tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous() or t.device != q0.device:
                        raise ValueError("out[%r] must be a contiguous float64 tensor of shape %s" % (key, shape))
                    setattr(gf, field, ptr(t))
                    grads.append(t)
                gf.gref_step_stride = 0 if sum_ref else q0.numel()
            ref = lambda x: C.byref(x) if x is not None else None
            if accumulate is None:
                check(lib().rdyn_rollout_adjoint_feedback(self._h, C.byref(b), C.byref(d), comps, n_comps, ref(ext), C.byref(g), ref(fb), ref(gf),
                                                          chunk_samples, None, 0))
                return (gq0, gdq0, gtau, status) + ((gext,) if want_ext else ()) + tuple(grads)
            law_grads = tuple(grads)
            nbytes = lib().rdyn_rollout_adjoint_feedback_parameters_workspace_bytes(self._h, C.byref(d), comps, n_comps, ref(ext), ref(fb), N,
                                                                                    chunk_samples)
        elif accumulate is None:
            nbytes = lib().rdyn_rollout_adjoint_workspace_bytes(self._h, C.byref(d), N, chunk_samples)
        else:
            nbytes = lib().rdyn_rollout_adjoint_parameters_workspace_bytes(self._h, C.byref(d), comps, n_comps, N, chunk_samples)
        if workspace is None and nbytes > 0:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q0.device)
        ws = (workspace.data_ptr() if workspace is not None else None, workspace.numel() if workspace is not None else 0)
        if accumulate is None:
            check(lib().rdyn_rollout_adjoint(self._h, C.byref(b), C.byref(d), comps, n_comps, chunk_samples, *ws))
            return gq0, gdq0, gtau, status
        sizes = {"gpi": 10 * self.getJointsNumber(), "gcomp": components.columns if components is not None else 0}
        grads = {}
        for key, size in sizes.items():
            t = out.get(key)
            if t is None:
                if accumulate and size:
                    raise ValueError("accumulate=True needs out['gpi'] (and out['gcomp'] with components)")
                t = torch.empty((size,), dtype=torch.float64, device=q0.device)
            elif tuple(t.shape) != (size,) or t.dtype != torch.float64 or not t.is_contiguous() or t.device != q0.device:
                raise ValueError("out[%r] must be a contiguous float64 tensor of %d entries" % (key, size))
            grads[key] = t
        pg = _lib.ParameterGradient(grads["gpi"].data_ptr(), ptr(grads["gcomp"]), 1 if accumulate else 0)
        gcomp = grads["gcomp"] if components is not None else None
        if wrenches is not None or closed is not None:
            check(lib().rdyn_rollout_adjoint_feedback_parameters(self._h, C.byref(b), C.byref(d), comps, n_comps, ref(ext), C.byref(g), ref(fb),
                                                                 ref(gf), C.byref(pg), chunk_samples, *ws))
            return (gq0, gdq0, gtau, grads["gpi"], gcomp, status) + law_grads
        check(lib().rdyn_rollout_adjoint_parameters(self._h, C.byref(b), C.byref(d), comps, n_comps, C.byref(pg), chunk_samples, *ws))
        return gq0, gdq0, gtau, grads["gpi"], gcomp, status

    def getRegressor(self, q, Dq, DDq, layout="sample", y_layout=None, out=None, tau_out=None, with_torque=False):
        """Regressor (and optionally the fused joint torque).

        y_layout: "per_sample" -> (N, P, n): Y[s] is the column-major n x P Eigen image (default for layout="sample");
                  "stacked"    -> (P, N*n):  column-major (N*n) x P, row = s*n + j;
                  "element"    -> (P, n, N): column-major (n*N) x P, row = j*N + s (default for layout="element").
        """
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, DDq)
        n, P = self.getActiveJointsNumber(), 10 * self.getJointsNumber()
        if y_layout is None:
            y_layout = "element" if lay == LAYOUT_ELEMENT_MAJOR else "per_sample"
        if y_layout == "per_sample":
            shape, yl = (N, P, n), RegressorLayout(n * P, 1, n)
        elif y_layout == "stacked":
            shape, yl = (P, N * n), RegressorLayout(n, 1, N * n)
        elif y_layout == "element":
            shape, yl = (P, n, N), RegressorLayout(1, N, n * N)
        else:
            raise ValueError("unknown y_layout %r" % (y_layout,))
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=q.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 tensor of shape %s" % (shape,))
        tau = None
        if with_torque or tau_out is not None:
            tau = self._out(q, N, lay, (n,), tau_out)
        check(lib().rdyn_regressor(self._h, C.byref(b), tau.data_ptr() if tau is not None else None, out.data_ptr(), C.byref(yl)))
        return (out, tau) if tau is not None else out


    def getRegressorGram(self, q, Dq, DDq, tau_meas=None, layout="sample", chunk_samples=0, out=None, accumulate=False,
                         workspace=None, packed_out=None):
        """Normal equations of the stacked regressor of this batch without leaving Y in HBM:
        returns (G = A^T A (P, P), c = A^T tau_meas (P,), bb = tau_meas^T tau_meas (1,)).  include/rdyn.h: rdyn_regressor_gram.
        packed_out: a (P*P + P + 2,) float64 buffer [G | c | bb | count] -- the all-reduce payload of the multi-GPU path; G, c, bb are
        written straight into it (the returned tensors are views), the count slot is the caller's (rosdyn_amd.gram.packed_buffer)."""
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, DDq)
        P = 10 * self.getJointsNumber()
        if tau_meas is not None and (tau_meas.shape != q.shape or tau_meas.dtype != torch.float64 or not tau_meas.is_contiguous()):
            raise ValueError("Input data dimensions mismatch")
        if packed_out is not None:
            if out is not None:
                raise ValueError("packed_out and out are exclusive")
            if packed_out.dtype != torch.float64 or packed_out.numel() != P * P + P + 2 or not packed_out.is_contiguous() or packed_out.device != q.device:
                raise ValueError("packed_out must be a contiguous float64 tensor of P*P + P + 2 elements on the batch's device")
            flat = packed_out.view(-1)
            out = (flat[:P * P].view(P, P), flat[P * P:P * P + P], flat[P * P + P:P * P + P + 1])
        if out is None:
            out = (torch.empty((P, P), dtype=torch.float64, device=q.device), torch.empty((P,), dtype=torch.float64, device=q.device),
                   torch.empty((1,), dtype=torch.float64, device=q.device))
            if accumulate:
                raise ValueError("accumulate needs out=")
        G, c, bb = out
        nbytes = lib().rdyn_regressor_gram_workspace_bytes(self._h, chunk_samples)
        if workspace is None:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        check(lib().rdyn_regressor_gram(self._h, C.byref(b), tau_meas.data_ptr() if tau_meas is not None else None,
                                        G.data_ptr(), c.data_ptr(), bb.data_ptr(), 1 if accumulate else 0, chunk_samples,
                                        workspace.data_ptr(), workspace.numel()))
        return G, c, bb

    def getRegressorGramWide(self, q, Dq, DDq, tau_meas=None, layout="sample", chunk_samples=0, out=None, accumulate=False,
                             workspace=None):
        """getRegressorGram for every chain the library ingests, up to 415 columns (include/rdyn.h: rdyn_regressor_gram_wide: chains
        with 12 to 32 input joints through the column-panel Gram; what getRegressorGram serves goes to it).
        Returns (G = A^T A (P, P), c = A^T tau_meas (P,), bb = tau_meas^T tau_meas (1,))."""
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, DDq)
        P = 10 * self.getJointsNumber()
        if tau_meas is not None and (tau_meas.shape != q.shape or tau_meas.dtype != torch.float64 or not tau_meas.is_contiguous()):
            raise ValueError("Input data dimensions mismatch")
        if out is None:
            out = (torch.empty((P, P), dtype=torch.float64, device=q.device), torch.empty((P,), dtype=torch.float64, device=q.device),
                   torch.empty((1,), dtype=torch.float64, device=q.device))
            if accumulate:
                raise ValueError("accumulate needs out=")
        G, c, bb = out
        nbytes = lib().rdyn_regressor_gram_wide_workspace_bytes(self._h, chunk_samples)
        if nbytes == 0:
            raise ValueError("rdyn_regressor_gram_wide: at most 415 columns")
        if workspace is None:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        check(lib().rdyn_regressor_gram_wide(self._h, C.byref(b), tau_meas.data_ptr() if tau_meas is not None else None,
                                             G.data_ptr(), c.data_ptr(), bb.data_ptr(), 1 if accumulate else 0, chunk_samples,
                                             workspace.data_ptr(), workspace.numel()))
        return G, c, bb

    def getIdentificationGramWide(self, components, q, Dq, DDq, tau_meas, layout="sample", chunk_samples=0, out=None,
                                  accumulate=False, workspace=None):
        """getIdentificationGram for every chain the library ingests, up to 415 columns of [Y | C] (include/rdyn.h:
        rdyn_identification_gram_wide).  Returns (G (P+K, P+K), c (P+K,), bb (1,))."""
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, DDq)
        if tau_meas.shape != q.shape or tau_meas.dtype != torch.float64 or not tau_meas.is_contiguous():
            raise ValueError("Input data dimensions mismatch")
        arr, n_comps = (C.cast(components._arr, C.c_void_p), components.n_comps) if components is not None else (None, 0)
        cols = 10 * self.getJointsNumber() + (components.columns if components is not None else 0)
        if out is None:
            out = (torch.empty((cols, cols), dtype=torch.float64, device=q.device), torch.empty((cols,), dtype=torch.float64, device=q.device),
                   torch.empty((1,), dtype=torch.float64, device=q.device))
            if accumulate:
                raise ValueError("accumulate needs out=")
        G, c, bb = out
        nbytes = lib().rdyn_identification_gram_wide_workspace_bytes(self._h, arr, n_comps, chunk_samples)
        if nbytes == 0:
            raise ValueError("rdyn_identification_gram_wide: at most 415 columns (regressor + components)")
        if workspace is None:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        check(lib().rdyn_identification_gram_wide(self._h, arr, n_comps, C.byref(b), tau_meas.data_ptr(), G.data_ptr(), c.data_ptr(),
                                                  bb.data_ptr(), 1 if accumulate else 0, chunk_samples, workspace.data_ptr(),
                                                  workspace.numel()))
        return G, c, bb

    def getRegressorTsqr(self, q, Dq, DDq, tau_meas=None, layout="sample", out=None, accumulate=False, workspace=None):
        """R factor of the stacked [regressor | tau_meas] of this batch WITHOUT forming A'A (include/rdyn.h: rdyn_regressor_tsqr,
        BASELINE.json configs[2]).  Returns R1 = [R d; 0 rho] as a (P + 1, P + 1) tensor in math layout (upper triangular)."""
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, DDq)
        P1 = 10 * self.getJointsNumber() + 1
        if tau_meas is not None and (tau_meas.shape != q.shape or tau_meas.dtype != torch.float64 or not tau_meas.is_contiguous()):
            raise ValueError("Input data dimensions mismatch")
        buf = torch.zeros((P1, P1), dtype=torch.float64, device=q.device) if out is None else out.t().contiguous()
        nbytes = lib().rdyn_regressor_tsqr_workspace_bytes(self._h)
        if nbytes == 0:
            raise ValueError("rdyn_regressor_tsqr: chains of 1..8 input joints in chain order, at most 112 columns after the reduction")
        if workspace is None:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        check(lib().rdyn_regressor_tsqr(self._h, C.byref(b), tau_meas.data_ptr() if tau_meas is not None else None, buf.data_ptr(),
                                        1 if accumulate else 0, workspace.data_ptr(), workspace.numel()))
        if out is not None:           # the C side is column-major: `buf` was a transposed copy of `out`
            out.copy_(buf.t())
            return out
        return buf.t()

    def getIdentificationGram(self, components, q, Dq, DDq, tau_meas, layout="sample", out=None, accumulate=False, workspace=None):
        """The identification step in one call (include/rdyn.h: rdyn_identification_gram): normal equations of [Y | C] with
        the measured torque; `components` is a rosdyn_amd.components.ComponentSet or None.  Returns (G (P+K, P+K), c (P+K,),
        bb (1,)); the unknowns are [the 10-per-link inertial parameters ; the components' parameters]."""
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, DDq)
        if tau_meas.shape != q.shape or tau_meas.dtype != torch.float64 or not tau_meas.is_contiguous():
            raise ValueError("Input data dimensions mismatch")
        arr, n_comps = (C.cast(components._arr, C.c_void_p), components.n_comps) if components is not None else (None, 0)
        cols = 10 * self.getJointsNumber() + (components.columns if components is not None else 0)
        if out is None:
            out = (torch.empty((cols, cols), dtype=torch.float64, device=q.device), torch.empty((cols,), dtype=torch.float64, device=q.device),
                   torch.empty((1,), dtype=torch.float64, device=q.device))
            if accumulate:
                raise ValueError("accumulate needs out=")
        G, c, bb = out
        nbytes = lib().rdyn_identification_gram_workspace_bytes(self._h, arr, n_comps)
        if nbytes == 0:
            raise ValueError("at most 111 columns (regressor + components) are supported")
        if workspace is None:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        check(lib().rdyn_identification_gram(self._h, arr, n_comps, C.byref(b), tau_meas.data_ptr(), G.data_ptr(), c.data_ptr(),
                                             bb.data_ptr(), 1 if accumulate else 0, workspace.data_ptr(), workspace.numel()))
        return G, c, bb


    def getIdentificationTsqr(self, components, q, Dq, DDq, tau_meas, layout="sample", out=None, accumulate=False, workspace=None):
        """R factor of the identification step's stacked [Y | C | tau_meas] WITHOUT forming the normal equations (include/rdyn.h:
        rdyn_identification_tsqr).  Returns R1 = [R d; 0 rho] as a (P + K + 1, P + K + 1) tensor in math layout (upper triangular);
        solve with rosdyn_amd.gram.solve_r_factor."""
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, DDq)
        if tau_meas.shape != q.shape or tau_meas.dtype != torch.float64 or not tau_meas.is_contiguous():
            raise ValueError("Input data dimensions mismatch")
        arr, n_comps = (C.cast(components._arr, C.c_void_p), components.n_comps) if components is not None else (None, 0)
        n1 = 10 * self.getJointsNumber() + (components.columns if components is not None else 0) + 1
        buf = torch.zeros((n1, n1), dtype=torch.float64, device=q.device) if out is None else out.t().contiguous()
        nbytes = lib().rdyn_identification_tsqr_workspace_bytes(self._h, arr, n_comps)
        if nbytes == 0:
            raise ValueError("rdyn_identification_tsqr: chains of 1..8 input joints in chain order, at most 112 columns after the reduction")
        if workspace is None:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        check(lib().rdyn_identification_tsqr(self._h, arr, n_comps, C.byref(b), tau_meas.data_ptr(), buf.data_ptr(), 1 if accumulate else 0,
                                             workspace.data_ptr(), workspace.numel()))
        R1 = buf.t()   # the library writes column-major
        if out is not None:
            out.copy_(R1)
            return out
        return R1


    def lastTsqrReport(self, n_samples, workspace, components=None):
        """What the last getRegressorTsqr / getIdentificationTsqr call that used `workspace` did (include/rdyn.h:
        rdyn_tsqr_last_report): dict(route = 0 Householder folds / 1 preconditioned CholeskyQR; stage = 0 accepted after round 0,
        1 after round 1, 2 the stand-by Householder factorisation ran; n_deferred; gamma, rho of the two rounds).  Synchronises."""
        from ._lib import RdynTsqrReport
        torch = _torch()
        arr, n_comps = (C.cast(components._arr, C.c_void_p), components.n_comps) if components is not None else (None, 0)
        rep = RdynTsqrReport()
        stream = torch.cuda.current_stream(workspace.device).cuda_stream
        check(lib().rdyn_tsqr_last_report(self._h, arr, n_comps, int(n_samples), workspace.data_ptr(), workspace.device.index or 0, stream,
                                          C.byref(rep)))
        return dict(route=rep.route, stage=rep.stage, n_deferred=rep.n_deferred, gamma=tuple(rep.gamma), rho=tuple(rep.rho))

    def getRegressorTsqrWide(self, q, Dq, DDq, tau_meas=None, layout="sample", chunk_samples=0, out=None, accumulate=False,
                             workspace=None):
        """getRegressorTsqr for up to 416 columns with tau_meas (include/rdyn.h: rdyn_regressor_tsqr_wide, column-panel CholeskyQR
        over chunk images; shapes the narrow call serves are handed to it).  Returns R1 as a (P + 1, P + 1) tensor in math layout."""
        return self._tsqr_wide(None, q, Dq, DDq, tau_meas, layout, chunk_samples, out, accumulate, workspace)

    def getIdentificationTsqrWide(self, components, q, Dq, DDq, tau_meas, layout="sample", chunk_samples=0, out=None, accumulate=False,
                                  workspace=None):
        """getIdentificationTsqr for up to 416 columns (include/rdyn.h: rdyn_identification_tsqr_wide).  Returns R1 as a
        (P + K + 1, P + K + 1) tensor in math layout; solve with rosdyn_amd.gram.solve_r_factor."""
        return self._tsqr_wide(components, q, Dq, DDq, tau_meas, layout, chunk_samples, out, accumulate, workspace)

    def _tsqr_wide(self, components, q, Dq, DDq, tau_meas, layout, chunk_samples, out, accumulate, workspace):
        torch = _torch()
        b, N, lay = self._batch(layout, q, Dq, DDq)
        if tau_meas is not None and (tau_meas.shape != q.shape or tau_meas.dtype != torch.float64 or not tau_meas.is_contiguous()):
            raise ValueError("Input data dimensions mismatch")
        arr, n_comps = (C.cast(components._arr, C.c_void_p), components.n_comps) if components is not None else (None, 0)
        n1 = 10 * self.getJointsNumber() + (components.columns if components is not None else 0) + 1
        buf = torch.zeros((n1, n1), dtype=torch.float64, device=q.device) if out is None else out.t().contiguous()
        if components is None:
            nbytes = lib().rdyn_regressor_tsqr_wide_workspace_bytes(self._h, int(chunk_samples))
        else:
            nbytes = lib().rdyn_identification_tsqr_wide_workspace_bytes(self._h, arr, n_comps, int(chunk_samples))
        if nbytes == 0:
            raise ValueError("the wide R factor serves at most 416 columns (with tau_meas)")
        if workspace is None:
            workspace = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
        tau = tau_meas.data_ptr() if tau_meas is not None else None
        if components is None:
            check(lib().rdyn_regressor_tsqr_wide(self._h, C.byref(b), tau, buf.data_ptr(), 1 if accumulate else 0, int(chunk_samples),
                                                 workspace.data_ptr(), workspace.numel()))
        else:
            check(lib().rdyn_identification_tsqr_wide(self._h, arr, n_comps, C.byref(b), tau, buf.data_ptr(), 1 if accumulate else 0,
                                                      int(chunk_samples), workspace.data_ptr(), workspace.numel()))
        if out is not None:           # the C side is column-major: `buf` was a transposed copy of `out`
            out.copy_(buf.t())
            return out
        return buf.t()

    def lastTsqrWideReport(self, workspace, components=None):
        """What the last getRegressorTsqrWide / getIdentificationTsqrWide call that used `workspace` did (include/rdyn.h:
        rdyn_tsqr_wide_last_report): dict(route = 2 column-panel CholeskyQR, 0 served by the narrow call -- see lastTsqrReport;
        stage = the accepted round 0..2, 3 none; n_deferred; gamma, rho of rounds 0..2).  Synchronises."""
        from .gram import tsqr_wide_last_report
        n1 = 10 * self.getJointsNumber() + (components.columns if components is not None else 0) + 1
        return tsqr_wide_last_report(n1, workspace)


def createChain(urdf_xml, base_frame, tool_frame, gravity=(0.0, 0.0, 0.0)):
    return Chain(urdf_xml, base_frame, tool_frame, gravity)
