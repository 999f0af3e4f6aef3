// rdyn_api_dynamics.cpp -- the forward-dynamics family of the C-ABI (include/rdyn.h): rdyn_forward_dynamics(_components),
// rdyn_rollout(_components), their forms with external link wrenches rdyn_forward_dynamics_ext and rdyn_rollout_ext, the closed loop
// rdyn_rollout_feedback and its model-based laws rdyn_rollout_model_feedback,
// rdyn_forward_dynamics_derivatives, rdyn_forward_dynamics_vjp, rdyn_rollout_adjoint, their parameter-gradient
// forms rdyn_forward_dynamics_parameter_vjp and rdyn_rollout_adjoint_parameters, their forms with external link wrenches
// rdyn_forward_dynamics_vjp_ext and rdyn_rollout_adjoint_ext, the adjoint of the closed loop rdyn_rollout_adjoint_feedback, and the
// workspace queries.
// Every entry runs check_batch and its own pointer / descriptor checks, then dyn_prepare (the checks and the set-up all of them share),
// then either one launch (chains the unrolled kernels sweep) or the chunked route through its workspace.  The workspace of every chunked
// route is described ONCE, by a *Layout struct: the query returns its total, the call carves its pointers from its offsets.
#include "rdyn_api_common.h"

// ---- the two routes ------------------------------------------------------------------------------------------------
// Chains the unrolled kernels sweep (long ones through their reduced companion, which has the same input joints, M and h): one launch,
// no workspace.  More than RDYN_MAX_SWEPT_JOINTS input joints: element-major chunk images [M | h] ((n n + n) doubles per sample)
// written by k_long_inertia and the wrench recursion, factorised and solved in place by k_fwd_solve; the default chunk is the rule of
// rdyn_regressor_gram_wide (an image within 128 MiB, at least 16 384 samples).
// With external wrenches (ext) every long chain takes the chunked route on the ORIGINAL chain: the wrenches belong to its links, which
// the reduced companion no longer has.
static bool fwd_dyn_by_chunks(const rdyn_chain* c, bool ext = false) { return c->long_chain() && (ext || !c->reduced); }
static int64_t fwd_dyn_chunk(const rdyn_chain* c, int64_t chunk_samples)
{
  const int64_t n = c->n_active();
  const int64_t fit = ((int64_t)128 << 20) / ((n * n + n) * (int64_t)sizeof(double)) & ~(int64_t)63;
  return chunk_samples > 0 ? chunk_samples : (fit > 16384 ? fit : 16384);
}

// ---- workspace layouts ---------------------------------------------------------------------------------------------
// Byte offsets from the start of the workspace, every region 256-byte aligned; total = 0: the call needs no workspace (a chain swept in
// registers, or arguments the call refuses anyway).  Each layout starts with the one it extends, so a pass of the smaller route runs
// in the front of the larger route's workspace.
namespace
{

// forward dynamics: the image [M | h] of `chunk` samples at offset 0
struct FwdLayout { int64_t chunk; size_t total; };
// derivatives: + the chunk's status words (the caller's status may be null; the column kernel needs them)
struct DerivLayout { FwdLayout f; size_t status, total; };
// product: + dddq_dq | dddq_dv | minv of one chunk, element-major, + the chunk's seeds (copied before the first pass: tau_bar may alias
// them, and when the caller wants no ddq an output array takes the pass's ddq)
struct VjpLayout { DerivLayout d; size_t Dq, Dv, Mi, seed, total; };
// the tail of the rollout and adjoint workspaces: `count` arrays of n N doubles in the batch's layout, `stride` bytes apart, then two
// int32 per sample (the pass's status, the running minimum)
struct StateLayout
{
  size_t first, stride, count, st_stage, st_run, total;
  double* array(void* workspace, size_t i) const { return i < count ? (double*)((char*)workspace + first + i * stride) : nullptr; }
};
// rollout: q | dq | ddq and for RK4 sq | sv | aq | av; the closed loop: + u, the command of the evaluation, behind them
struct RolloutLayout { FwdLayout f; StateLayout s; };
// adjoint: lq | lv | mu | qb | vb | tb and for RK4 xq | xv | kq | kv | gt | x2q | x2v | x3q | x3v | x4q | x4v | acc
struct AdjointLayout { VjpLayout v; StateLayout s; };

static FwdLayout fwd_layout(const rdyn_chain* c, int64_t chunk_samples, bool ext = false)
{
  FwdLayout L = {};
  if (!c || c->n_active() < 1 || chunk_samples < 0 || !fwd_dyn_by_chunks(c, ext)) return L;
  const size_t n = (size_t)c->n_active();
  L.chunk = fwd_dyn_chunk(c, chunk_samples);
  L.total = align256((size_t)L.chunk * (n * n + n) * sizeof(double));
  return L;
}

static DerivLayout deriv_layout(const rdyn_chain* c, int64_t chunk_samples)
{
  DerivLayout L = {};
  L.f = fwd_layout(c, chunk_samples);
  if (!L.f.total) return L;
  L.status = L.f.total;
  L.total = L.status + align256((size_t)L.f.chunk * sizeof(int32_t));
  return L;
}

static VjpLayout vjp_layout(const rdyn_chain* c, int64_t chunk_samples)
{
  VjpLayout L = {};
  L.d = deriv_layout(c, chunk_samples);
  if (!L.d.total) return L;
  const size_t n = (size_t)c->n_active();
  const size_t matrix = align256((size_t)L.d.f.chunk * n * n * sizeof(double));
  L.Dq = L.d.total;
  L.Dv = L.Dq + matrix;
  L.Mi = L.Dv + matrix;
  L.seed = L.Mi + matrix;
  L.total = L.seed + align256((size_t)L.d.f.chunk * n * sizeof(double));
  return L;
}

// behind a workspace of `first` bytes (0: no workspace at all)
static StateLayout state_layout(size_t first, size_t count, const rdyn_chain* c, int64_t n_samples)
{
  StateLayout s = {};
  if (!first) return s;
  s.first = first;
  s.stride = align256((size_t)n_samples * (size_t)c->n_active() * sizeof(double));
  s.count = count;
  s.st_stage = first + count * s.stride;
  s.st_run = s.st_stage + align256((size_t)n_samples * sizeof(int32_t));
  s.total = s.st_run + align256((size_t)n_samples * sizeof(int32_t));
  return s;
}

static RolloutLayout rollout_layout(const rdyn_chain* c, const rdyn_rollout_desc* d, int64_t n_samples, int64_t chunk_samples, bool ext = false,
                                    bool fb = false)
{
  RolloutLayout L = {};
  if (!d || n_samples < 0) return L;
  L.f = fwd_layout(c, chunk_samples, ext);
  L.s = state_layout(L.f.total, (d->integrator == RDYN_INTEGRATOR_RK4 ? 7 : 3) + (fb ? 1 : 0), c, n_samples);
  return L;
}

static AdjointLayout adjoint_layout(const rdyn_chain* c, const rdyn_rollout_adjoint_desc* d, int64_t n_samples, int64_t chunk_samples)
{
  AdjointLayout L = {};
  if (!d || n_samples < 0) return L;
  L.v = vjp_layout(c, chunk_samples);
  L.s = state_layout(L.v.total, d->integrator == RDYN_INTEGRATOR_RK4 ? 18 : 6, c, n_samples);
  return L;
}

// ---- what the entries share ----------------------------------------------------------------------------------------
static int refuse(const char* who, const char* what)
{
  rdyn_set_error("%s: %s", who, what);
  return RDYN_ERR_INVALID_ARGUMENT;
}

// What a call has in hand once dyn_prepare let it through
struct DynCall
{
  bool run;                      // false: no samples -- the call is done
  DeviceGuard guard;             // the batch's device is current until the call returns
  hipStream_t stream;
  int n;                         // input joints
  int64_t in_ss, in_sj;          // strides of the batch's n-vectors
  const rdyn_chain* sw;          // the chain the register kernels sweep and its constants on the device; null: the chunked route
  const RdynChainConst* chain;
  RdynComponentTable table;      // the component list, validated and sanitised (fill_components)
  const RdynComponentTable* comps;  // &table, or null without components: the chunked route then takes the plain solve kernel
};

// The checks every entry makes after check_batch and its own pointer / descriptor checks, in this order, and the set-up behind them:
// the sign of chunk_samples, the workspace against `need` (the total of the entry's layout), the component list; then no samples = done;
// the device, the strides, the swept chain or the chunked route (ext: the call has external wrenches).  who = the entry point (error texts).
static int dyn_prepare(const rdyn_chain* c, const rdyn_batch* b, const rdyn_component* comps, int n_comps, int64_t chunk_samples, size_t need,
                       const void* workspace, size_t workspace_bytes, const char* who, DynCall* k, bool ext = false)
{
  k->run = false;
  if (chunk_samples < 0) return refuse(who, "negative chunk_samples");
  if (b->n_samples > 0 && need > 0 && (!workspace || workspace_bytes < need))
  {
    rdyn_set_error("%s: workspace too small (%zu < %zu bytes)", who, workspace ? workspace_bytes : (size_t)0, need);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  k->n = c->n_active();
  memset(&k->table, 0, sizeof k->table);
  if (n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps))
  {
    rdyn_set_error("%s: 0..%d components, a list when there are any", who, RDYN_MAX_COMPONENTS);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  RdynComponentArgs a;
  memset(&a, 0, sizeof a);
  int st = fill_components(comps, n_comps, k->n, &a);
  if (st != RDYN_OK) return st;
  k->table.n_comps = n_comps;
  for (int i = 0; i < n_comps; ++i) k->table.comps[i] = a.comps[i];
  k->comps = n_comps ? &k->table : nullptr;
  if (b->n_samples == 0 || k->n < 1) return RDYN_OK;
  st = k->guard.enter(b->device);
  if (st != RDYN_OK) return st;
  k->stream = (hipStream_t)b->stream;
  rec_strides(b, k->n, &k->in_ss, &k->in_sj);
  k->sw = fwd_dyn_by_chunks(c, ext) ? nullptr : (c->long_chain() ? c->reduced.get() : c);
  k->run = true;
  return k->sw ? device_const(k->sw, &k->chain) : RDYN_OK;
}

// records of the drop-in layout leave through the wave's LDS tile in whole lines (rdyn_record_stage.h) when every one of these outputs
// (null: not asked for) starts on a line
template <class... P>
static bool stage_records(const rdyn_batch* b, P... out)
{
  return b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(out...);
}

// the descriptor fields a rollout and its adjoint share
static int check_integration(int n_steps, double dt, int integrator, const double* tau, const char* who)
{
  if (n_steps < 0 || !std::isfinite(dt) || dt == 0.0 || (integrator != RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER && integrator != RDYN_INTEGRATOR_RK4))
    return refuse(who, "negative n_steps, a step size that is zero or not finite, or an unknown integrator");
  if (n_steps > 0 && !tau) return refuse(who, "null torque pointer");
  return RDYN_OK;
}

// The external wrenches of a call: x.w null = none (ext null or ext->w null: the call IS the components call).  The link index, and for
// rollouts the step stride against one step's record; the strides of a record in the batch's layout.
static int check_ext(const rdyn_chain* c, const rdyn_batch* b, const rdyn_ext_wrenches* ext, bool steps, const char* who, RdynExtArgs* x)
{
  memset(x, 0, sizeof *x);
  if (!ext || !ext->w) return RDYN_OK;
  if (ext->link < -1 || ext->link > c->n_joints())
  {
    rdyn_set_error("%s: wrench link %d outside -1 .. %d (-1 = every link, %d = the tool)", who, (int)ext->link, c->n_joints(), c->n_joints());
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  const int64_t rec = ext->link < 0 ? 6 * (int64_t)(c->n_joints() + 1) : 6;
  if (steps && (ext->step_stride < 0 || (ext->step_stride != 0 && ext->step_stride < rec * b->n_samples)))
  {
    rdyn_set_error("%s: wrench step_stride %lld is negative, or not zero and smaller than one step's record (%lld doubles)", who,
                   (long long)ext->step_stride, (long long)(rec * b->n_samples));
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  x->w = ext->w;
  rec_strides(b, rec, &x->ss, &x->se);
  x->step = steps ? ext->step_stride : 0;
  x->one = ext->link < 0 ? 0 : 1 + ext->link;
  return RDYN_OK;
}

// reverse mode with wrenches serves the chains swept in registers on their own links; every chain whose rdyn_forward_dynamics_ext takes
// the chunked route is refused
static int ext_reverse_refusal(const rdyn_chain* c, const char* who)
{
  if (!fwd_dyn_by_chunks(c, true)) return RDYN_OK;
  rdyn_set_error("%s: with external wrenches, chains that rdyn_forward_dynamics_ext serves by its chunked route (more than %d input joints, "
                 "or more than %d chain joints on a reduced companion; this chain has %d input joints, %d chain joints) are not served yet; "
                 "without wrenches the call serves them",
                 who, RDYN_MAX_SWEPT_JOINTS, RDYN_MAX_SWEPT_JOINTS, c->n_active(), c->n_joints());
  return RDYN_ERR_UNSUPPORTED;
}

}  // namespace

int long_deriv_lds_refusal(const rdyn_chain* c, const char* who)
{
  if (rdyn_long_torque_deriv_lanes(c->n_joints()) != 0) return RDYN_OK;
  rdyn_set_error("%s: the per-joint state of a chain of %d joints (%zu bytes for 16 samples) exceeds the LDS a workgroup may use on this device",
                 who, c->n_joints(), rdyn_long_torque_deriv_lds_bytes(c->n_joints(), 16));
  return RDYN_ERR_UNSUPPORTED;
}

// ---- forward dynamics: ddq = M^-1 (tau - h) (rdyn_fwd_dyn.hip) -------------------------------------------------
// one pass of the chunked route over n_samples samples: per chunk the image [M | h] (k_long_inertia, the wrench recursion), then k_fwd_solve
// (comps: null = the plain solve kernel; otherwise its variant, which subtracts tau_c at the sample's (q, dq) from tau; ext: null, or the
// wrenches of the pass (ext->w at the first sample): the wrench recursion takes them and writes h + tau_E where it writes h, tau_E being
// linear in ext and independent of dq -- no second launch, no buffer)
static int fwd_dyn_chunks(const rdyn_chain* c, const double* q, const double* dq, const double* tau, double* ddq, int32_t* status,
                          int64_t n_samples, int64_t in_ss, int64_t in_sj, int64_t chunk, double* image, hipStream_t stream,
                          const RdynComponentTable* comps, const RdynExtArgs* ext = nullptr)
{
  const int n = c->n_active();
  RdynLongLocalArgs ia;
  memset(&ia, 0, sizeof ia);
  int st = device_const_long(c, &ia.chain_long);
  if (st != RDYN_OK) return st;
  RdynKinExtArgs ha;
  memset(&ha, 0, sizeof ha);
  ha.chain_long = ia.chain_long;
  for (int64_t s0 = 0; s0 < n_samples; s0 += chunk)
  {
    const int64_t cnt = (n_samples - s0 < chunk) ? n_samples - s0 : chunk;
    ia.q = q + s0 * in_ss;
    ia.n_samples = cnt;
    ia.in_ss = in_ss;
    ia.in_sj = in_sj;
    ia.n_active = n;
    ia.M = image;
    ia.m_ss = 1;
    ia.m_se = cnt;
    RDYN_HIP_TRY(rdyn_launch_long_local(RDYN_MODE_INERTIA, c->n_joints(), ia, stream));
    ha.q = ia.q;
    ha.dq = dq + s0 * in_ss;
    ha.n_samples = cnt;
    ha.in_ss = in_ss;
    ha.in_sj = in_sj;
    ha.tau = image + (int64_t)n * n * cnt;
    ha.tau_ss = 1;
    ha.tau_sj = cnt;
    if (ext)
    {
      ha.ext = ext->w + s0 * ext->ss;
      ha.ext_ss = ext->ss;
      ha.ext_se = ext->se;
      ha.ext_one = ext->one;
    }
    RDYN_HIP_TRY(rdyn_launch_long_ext(c->n_joints(), ha, stream));
    RdynFwdSolveArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.image = image;
    sa.ld = cnt;
    sa.n = n;
    sa.tau = tau + s0 * in_ss;
    sa.ddq = ddq + s0 * in_ss;
    sa.status = status ? status + s0 : nullptr;
    sa.n_samples = cnt;
    sa.in_ss = in_ss;
    sa.in_sj = in_sj;
    if (!comps)
    {
      RDYN_HIP_TRY(rdyn_launch_forward_solve(sa, stream));
      continue;
    }
    RdynFwdSolveCompArgs sc;
    sc.s = sa;
    sc.q = ia.q;
    sc.dq = ha.dq;
    sc.t = *comps;
    RDYN_HIP_TRY(rdyn_launch_forward_solve_components(sc, stream));
  }
  return RDYN_OK;
}

// who = the entry point (error texts); comps with n_comps = 0 is the plain call: the same kernels; ext null, or without w: no wrenches,
// the same kernels again
static int forward_dynamics(const rdyn_chain* c, const rdyn_batch* b, const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext,
                            const double* tau, double* ddq, int32_t* status, int64_t chunk_samples, void* workspace, size_t workspace_bytes,
                            const char* who)
{
  int st = check_batch(c, b, true, false, who, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (b->n_samples > 0 && (!tau || !ddq)) return refuse(who, "null torque or acceleration pointer");
  RdynExtArgs x;
  st = check_ext(c, b, ext, false, who, &x);
  if (st != RDYN_OK) return st;
  const FwdLayout L = fwd_layout(c, chunk_samples, x.w != nullptr);
  DynCall k;
  st = dyn_prepare(c, b, comps, n_comps, chunk_samples, L.total, workspace, workspace_bytes, who, &k, x.w != nullptr);
  if (st != RDYN_OK || !k.run) return st;
  if (!k.sw)
    return fwd_dyn_chunks(c, b->q, b->dq, tau, ddq, status, b->n_samples, k.in_ss, k.in_sj, L.chunk, (double*)workspace, k.stream, k.comps,
                          x.w ? &x : nullptr);
  RdynFwdDynArgs a;
  memset(&a, 0, sizeof a);
  a.chain = k.chain;
  a.q = b->q;
  a.dq = b->dq;
  a.tau = tau;
  a.ddq = ddq;
  a.status = status;
  a.n_samples = b->n_samples;
  a.in_ss = k.in_ss;
  a.in_sj = k.in_sj;
  a.staged = stage_records(b, ddq) ? k.n : 0;
  if (x.w)
  {
    RdynFwdDynExtArgs ae;
    ae.c.f = a;
    ae.c.t = k.table;
    ae.x = x;
    RDYN_HIP_TRY(rdyn_launch_forward_dynamics_ext(k.sw->n_joints(), ae, k.stream));
    return RDYN_OK;
  }
  if (n_comps == 0)
  {
    RDYN_HIP_TRY(rdyn_launch_forward_dynamics(k.sw->n_joints(), a, k.stream));
    return RDYN_OK;
  }
  RdynFwdDynCompArgs ac;
  ac.f = a;
  ac.t = k.table;
  RDYN_HIP_TRY(rdyn_launch_forward_dynamics_components(k.sw->n_joints(), ac, k.stream));
  return RDYN_OK;
}

// ---- rollouts: T integrator steps of the forward dynamics (rdyn_rollout.hip) ------------------------------------
// Chains the unrolled kernels sweep: one launch for the whole horizon.  More input joints: per stage the chunked forward dynamics above,
// then k_rollout_stage on the state arrays of RolloutLayout.
// who = the entry point (error texts); comps with n_comps = 0 is the plain call: the same kernels; ext null, or without w: no wrenches;
// fb null: open loop.  Otherwise the closed loop (rdyn_rollout_fb.hip): one launch of k_rollout_fb, or on the chunked route
// k_rollout_command before the pass of every evaluation whose command is formed anew (hold: the step's first), the pass taking the command
// array of the workspace where it took tau_t.
// mfb null: the PD law.  Otherwise a model-based law (rdyn_rollout_fb_model.hip): the chains swept in registers only, one launch of
// k_rollout_fb_model, which sweeps the model chain (its reduced companion where the plant's is swept) where the command is formed.
static bool model_feedback_by_chunks(const rdyn_chain* c, const rdyn_ext_wrenches* ext) { return fwd_dyn_by_chunks(c, ext && ext->w); }

static int rollout(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_desc* d, const rdyn_component* comps, int n_comps,
                   const rdyn_ext_wrenches* ext, int64_t chunk_samples, void* workspace, size_t workspace_bytes, const char* who,
                   const rdyn_feedback* fb = nullptr, const rdyn_model_feedback* mfb = nullptr)
{
  int st = check_batch(c, b, true, false, who, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!d) return refuse(who, "null descriptor");
  const int n = c->n_active();
  const int64_t N = b->n_samples;
  st = check_integration(d->n_steps, d->dt, d->integrator, d->tau, who);
  if (st != RDYN_OK) return st;
  double* const tau_traj = fb ? fb->tau_traj : nullptr;
  const bool traj = d->q_traj || d->dq_traj || tau_traj;
  if (N > 0 && !d->q_end && !d->dq_end && !traj) return refuse(who, "every output is null");
  if (traj && (d->traj_every < 1 || d->traj_step_stride < (int64_t)n * N))
    return refuse(who, "a trajectory needs traj_every >= 1 and traj_step_stride >= n * n_samples");
  RdynExtArgs x;
  st = check_ext(c, b, ext, true, who, &x);
  if (st != RDYN_OK) return st;
  if (fb)
  {
    if (!fb->q_ref || !fb->kp) return refuse(who, "null reference (q_ref) or gain (kp) pointer");
    if (fb->ref_step_stride < 0 || (fb->ref_step_stride != 0 && fb->ref_step_stride < (int64_t)n * N))
    {
      rdyn_set_error("%s: ref_step_stride %lld is negative, or not zero and smaller than one step's record (%lld doubles)", who,
                     (long long)fb->ref_step_stride, (long long)((int64_t)n * N));
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    if ((fb->hold != 0 && fb->hold != 1) || (fb->gains_per_sample != 0 && fb->gains_per_sample != 1))
      return refuse(who, "hold and gains_per_sample are 0 or 1");
  }
  const rdyn_chain* model_sw = nullptr;  // the model chain the law sweeps
  if (mfb)
  {
    if (!fb) return refuse(who, "a model-based law (mfb) without the feedback (fb) that holds its references and gains");
    const rdyn_chain* const m = mfb->model;
    if (!m) return refuse(who, "null model chain");
    if (mfb->law != RDYN_LAW_GRAVITY_COMPENSATION && mfb->law != RDYN_LAW_COMPUTED_TORQUE)
    {
      rdyn_set_error("%s: unknown law %d (gravity compensation is %d, computed torque %d)", who, (int)mfb->law,
                     (int)RDYN_LAW_GRAVITY_COMPENSATION, (int)RDYN_LAW_COMPUTED_TORQUE);
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    if (mfb->law == RDYN_LAW_GRAVITY_COMPENSATION && mfb->ddq_ref)
      return refuse(who, "ddq_ref belongs to the computed-torque law: gravity compensation takes none");
    if (m->n_joints() != c->n_joints())
    {
      rdyn_set_error("%s: the model has %d chain joints, the chain %d", who, m->n_joints(), c->n_joints());
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    for (int j = 0; j < c->n_joints(); ++j)
      if (m->host_joints[(size_t)j].type != c->host_joints[(size_t)j].type)
      {
        rdyn_set_error("%s: chain joint %d of the model is of another type than the chain's", who, j);
        return RDYN_ERR_INVALID_ARGUMENT;
      }
    if (m->active != c->active) return refuse(who, "the model's input joints differ from the chain's in selection or order");
    if (model_feedback_by_chunks(c, ext))
    {
      rdyn_set_error("%s: chains that rdyn_rollout_feedback serves by its chunked route (more than %d input joints, or with external wrenches "
                     "more than %d chain joints; this chain has %d input joints, %d chain joints) are not served with a model-based law: the "
                     "law is swept in registers",
                     who, RDYN_MAX_SWEPT_JOINTS, RDYN_MAX_SWEPT_JOINTS, n, c->n_joints());
      return RDYN_ERR_UNSUPPORTED;
    }
    const rdyn_chain* const sw = c->long_chain() ? c->reduced.get() : c;
    model_sw = m->long_chain() ? m->reduced.get() : m;
    if (!model_sw || model_sw->n_joints() != sw->n_joints())
      return refuse(who, "the model's swept chain (its reduced companion) has another joint count than the chain's");
  }
  const RolloutLayout L = rollout_layout(c, d, N, chunk_samples, x.w != nullptr, fb != nullptr);
  DynCall k;
  st = dyn_prepare(c, b, comps, n_comps, chunk_samples, mfb ? 0 : L.s.total, workspace, workspace_bytes, who, &k, x.w != nullptr);
  if (st != RDYN_OK || !k.run) return st;
  const int every = traj ? d->traj_every : 0;
  if (k.sw)
  {
    RdynRolloutArgs a;
    memset(&a, 0, sizeof a);
    a.chain = k.chain;
    a.q = b->q;
    a.dq = b->dq;
    a.tau = d->tau;
    a.tau_step = d->tau_step_stride;
    a.q_end = d->q_end;
    a.dq_end = d->dq_end;
    a.q_traj = d->q_traj;
    a.dq_traj = d->dq_traj;
    a.traj_step = d->traj_step_stride;
    a.status = d->status;
    a.n_samples = N;
    a.in_ss = k.in_ss;
    a.in_sj = k.in_sj;
    a.dt = d->dt;
    a.n_steps = d->n_steps;
    a.traj_every = every;
    a.integrator = d->integrator;
    a.n_active = n;
    // whole lines: every record of the kind starts on a line (the trajectory's step stride keeps the alignment of its first record)
    if ((d->q_end || d->dq_end) && stage_records(b, d->q_end, d->dq_end)) a.staged |= 1;
    if (traj && stage_records(b, d->q_traj, d->dq_traj, tau_traj) && (d->traj_step_stride * (int64_t)sizeof(double)) % 128 == 0) a.staged |= 2;
    if (fb)
    {
      RdynRolloutFbArgs af;
      memset(&af, 0, sizeof af);
      af.e.c.r = a;
      af.e.c.t = k.table;
      af.e.x = x;
      af.f.q_ref = fb->q_ref;
      af.f.dq_ref = fb->dq_ref;
      af.f.ref_step = fb->ref_step_stride;
      af.f.kp = fb->kp;
      af.f.kd = fb->kd;
      af.f.lim = fb->tau_limit;
      af.f.tau_traj = tau_traj;
      af.f.per_sample = fb->gains_per_sample;
      af.f.hold = fb->hold;
      if (mfb)
      {
        RdynRolloutModelFbArgs am;
        memset(&am, 0, sizeof am);
        am.b = af;
        st = device_const(model_sw, &am.m.model);
        if (st != RDYN_OK) return st;
        am.m.ddq_ref = mfb->ddq_ref;
        am.m.law = mfb->law;
        RDYN_HIP_TRY(rdyn_launch_rollout_model_feedback(k.sw->n_joints(), am, k.stream));
        return RDYN_OK;
      }
      RDYN_HIP_TRY(rdyn_launch_rollout_feedback(k.sw->n_joints(), af, k.stream));
      return RDYN_OK;
    }
    if (x.w)
    {
      RdynRolloutExtArgs ae;
      ae.c.r = a;
      ae.c.t = k.table;
      ae.x = x;
      RDYN_HIP_TRY(rdyn_launch_rollout_ext(k.sw->n_joints(), ae, k.stream));
      return RDYN_OK;
    }
    if (n_comps == 0)
    {
      RDYN_HIP_TRY(rdyn_launch_rollout(k.sw->n_joints(), a, k.stream));
      return RDYN_OK;
    }
    RdynRolloutCompArgs ac;
    ac.r = a;
    ac.t = k.table;
    RDYN_HIP_TRY(rdyn_launch_rollout_components(k.sw->n_joints(), ac, k.stream));
    return RDYN_OK;
  }
  const int64_t count = (int64_t)n * N;
  int32_t* const st_stage = (int32_t*)((char*)workspace + L.s.st_stage);
  int32_t* const st_run = (int32_t*)((char*)workspace + L.s.st_run);
  double *const q = L.s.array(workspace, 0), *const dq = L.s.array(workspace, 1), *const ddq = L.s.array(workspace, 2);
  const bool rk4 = d->integrator == RDYN_INTEGRATOR_RK4;  // (Euler has no stage arrays: with the closed loop, array 3 is the command)
  double *const sq = rk4 ? L.s.array(workspace, 3) : nullptr, *const sv = rk4 ? L.s.array(workspace, 4) : nullptr;
  RdynRolloutCopyArgs ca;
  memset(&ca, 0, sizeof ca);
  ca.q_src = b->q;
  ca.dq_src = b->dq;
  ca.q_dst = q;
  ca.dq_dst = dq;
  ca.st_dst = st_run;
  ca.count = count;
  ca.n_samples = N;
  RDYN_HIP_TRY(rdyn_launch_rollout_copy(ca, k.stream));
  RdynRolloutStageArgs sa;
  memset(&sa, 0, sizeof sa);
  sa.q = q;
  sa.dq = dq;
  sa.sq = sq;
  sa.sv = sv;
  sa.aq = rk4 ? L.s.array(workspace, 5) : nullptr;
  sa.av = rk4 ? L.s.array(workspace, 6) : nullptr;
  sa.ddq = ddq;
  sa.st_stage = st_stage;
  sa.st_run = st_run;
  sa.count = count;
  sa.n_samples = N;
  sa.n = n;
  sa.element_major = b->layout == RDYN_LAYOUT_ELEMENT_MAJOR;
  sa.integrator = d->integrator;
  sa.dt = d->dt;
  const int stages = d->integrator == RDYN_INTEGRATOR_RK4 ? 4 : 1;
  RdynRolloutCommandArgs fa;
  memset(&fa, 0, sizeof fa);
  if (fb)
  {
    fa.kp = fb->kp;
    fa.kd = fb->kd;
    fa.lim = fb->tau_limit;
    fa.u = L.s.array(workspace, L.s.count - 1);
    fa.st_run = st_run;
    fa.count = count;
    fa.n_samples = N;
    fa.n = n;
    fa.element_major = sa.element_major;
    fa.per_sample = fb->gains_per_sample;
  }
  for (int t = 0; t < d->n_steps; ++t)
  {
    const double* const tau_ff = d->tau + (int64_t)t * d->tau_step_stride;
    const double* const tau_t = fb ? fa.u : tau_ff;  // what the passes of the step take as their torques
    RdynExtArgs xt = x;  // the step's wrenches, held over its stages
    if (x.w) xt.w = x.w + (int64_t)t * x.step;
    const bool due = every > 0 && (t + 1) % every == 0;
    const int64_t rec = due ? ((t + 1) / every - 1) * d->traj_step_stride : 0;
    for (int stage = 0; stage < stages; ++stage)
    {
      if (fb && (stage == 0 || !fb->hold))
      {
        fa.q = stage ? sq : q;
        fa.dq = stage ? sv : dq;
        fa.tau_ff = tau_ff;
        fa.q_ref = fb->q_ref + (int64_t)t * fb->ref_step_stride;
        fa.dq_ref = fb->dq_ref ? fb->dq_ref + (int64_t)t * fb->ref_step_stride : nullptr;
        fa.rec = (stage == 0 && due && tau_traj) ? tau_traj + rec : nullptr;
        RDYN_HIP_TRY(rdyn_launch_rollout_command(fa, k.stream));
      }
      st = fwd_dyn_chunks(c, stage ? sq : q, stage ? sv : dq, tau_t, ddq, st_stage, N, k.in_ss, k.in_sj, L.f.chunk, (double*)workspace, k.stream,
                          k.comps, x.w ? &xt : nullptr);  // components and wrenches see the stage state
      if (st != RDYN_OK) return st;
      const bool last = stage == stages - 1;
      sa.stage = stage;
      sa.q_rec = (last && due && d->q_traj) ? d->q_traj + rec : nullptr;
      sa.dq_rec = (last && due && d->dq_traj) ? d->dq_traj + rec : nullptr;
      RDYN_HIP_TRY(rdyn_launch_rollout_stage(sa, k.stream));
    }
  }
  memset(&ca, 0, sizeof ca);
  ca.q_src = q;
  ca.dq_src = dq;
  ca.q_dst = d->q_end;
  ca.dq_dst = d->dq_end;
  ca.st_src = st_run;
  ca.st_dst = d->status;
  ca.count = count;
  ca.n_samples = N;
  RDYN_HIP_TRY(rdyn_launch_rollout_copy(ca, k.stream));
  return RDYN_OK;
}

// ---- derivatives of the forward dynamics: dDDq/dq, dDDq/dDq, M^-1 (rdyn_fwd_dyn_deriv.hip) ----------------------
// Chains the unrolled kernels sweep (long ones through their reduced companion): one launch, no workspace.  More input joints: per chunk
// the pass of the chunked forward dynamics (it leaves the factor of M in the image and ddq), k_long_torque_deriv at that ddq straight
// into the caller's matrices, k_fwd_solve_columns on them in place.
// the chunked route over n_samples samples (status may be null: st_chunk, one word per sample of a chunk, stands in; comps null = no
// components)
static int fwd_dyn_deriv_chunks(const rdyn_chain* c, const double* q_all, const double* dq_all, const double* tau, double* ddq, double* dddq_dq,
                                double* dddq_dv, double* minv, int32_t* status, int32_t* st_chunk, int64_t n_samples, int64_t in_ss,
                                int64_t in_sj, int64_t m_ss, int64_t m_se, int64_t chunk, double* image, const RdynComponentTable* comps,
                                hipStream_t stream)
{
  const int n = c->n_active();
  int st;
  RdynTorqueDerivArgs ta;
  memset(&ta, 0, sizeof ta);
  if (dddq_dq || dddq_dv)
  {
    st = device_const_long(c, &ta.chain_long);
    if (st != RDYN_OK) return st;
  }
  for (int64_t s0 = 0; s0 < n_samples; s0 += chunk)
  {
    const int64_t cnt = (n_samples - s0 < chunk) ? n_samples - s0 : chunk;
    const double* const q = q_all + s0 * in_ss;
    const double* const dq = dq_all + s0 * in_ss;
    double* const ddq_c = ddq + s0 * in_ss;
    int32_t* const st_c = status ? status + s0 : st_chunk;
    st = fwd_dyn_chunks(c, q, dq, tau + s0 * in_ss, ddq_c, st_c, cnt, in_ss, in_sj, chunk, image, stream, comps);
    if (st != RDYN_OK) return st;
    if (dddq_dq || dddq_dv)
    {
      ta.q = q;
      ta.dq = dq;
      ta.ddq = ddq_c;
      ta.n_samples = cnt;
      ta.in_ss = in_ss;
      ta.in_sj = in_sj;
      ta.dtau_dq = dddq_dq ? dddq_dq + s0 * m_ss : nullptr;
      ta.dtau_dv = dddq_dv ? dddq_dv + s0 * m_ss : nullptr;
      ta.m_ss = m_ss;
      ta.m_se = m_se;
      RDYN_HIP_TRY(rdyn_launch_long_torque_derivatives(c->n_joints(), ta, stream));
    }
    RdynFwdSolveColumnsArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.image = image;
    ca.ld = cnt;
    ca.n = n;
    ca.status = st_c;
    ca.q = q;
    ca.dq = dq;
    ca.n_samples = cnt;
    ca.in_ss = in_ss;
    ca.in_sj = in_sj;
    ca.dddq_dq = dddq_dq ? dddq_dq + s0 * m_ss : nullptr;
    ca.dddq_dv = dddq_dv ? dddq_dv + s0 * m_ss : nullptr;
    ca.minv = minv ? minv + s0 * m_ss : nullptr;
    ca.m_ss = m_ss;
    ca.m_se = m_se;
    if (comps) ca.t = *comps;
    RDYN_HIP_TRY(rdyn_launch_forward_solve_columns(ca, stream));
  }
  return RDYN_OK;
}

// ---- reverse-mode product of the forward dynamics (rdyn_fwd_dyn_vjp.hip) -----------------------------------------
// Chains the unrolled kernels sweep (long ones through their reduced companion): one launch, no workspace.  More input joints: per chunk
// the chunked route of the derivative call into the element-major matrices of VjpLayout, then k_vjp_products.
// the chunked route over n_samples samples; at least one of q_bar, dq_bar, tau_bar; status and ddq may be null
static int vjp_chunks(const rdyn_chain* c, const double* q, const double* dq, const double* tau, const double* ddq_bar, double* q_bar,
                      double* dq_bar, double* tau_bar, double* ddq, int32_t* status, int64_t n_samples, int64_t in_ss, int64_t in_sj,
                      const VjpLayout& L, void* workspace, const RdynComponentTable* comps, hipStream_t stream)
{
  const int n = c->n_active();
  const int64_t chunk = L.d.f.chunk;
  char* const p = (char*)workspace;
  double* const image = (double*)p;
  int32_t* const st_chunk = (int32_t*)(p + L.d.status);
  double* const Dq = (double*)(p + L.Dq);
  double* const Dv = (double*)(p + L.Dv);
  double* const Mi = (double*)(p + L.Mi);
  double* const seed = (double*)(p + L.seed);
  double* const ddq_pass = ddq ? ddq : (q_bar ? q_bar : (dq_bar ? dq_bar : tau_bar));  // (overwritten by the products of the same chunk)
  for (int64_t s0 = 0; s0 < n_samples; s0 += chunk)
  {
    const int64_t cnt = (n_samples - s0 < chunk) ? n_samples - s0 : chunk;
    const int64_t o = s0 * in_ss;
    int32_t* const st_c = status ? status + s0 : st_chunk;
    RDYN_HIP_TRY(rdyn_launch_vjp_seed_copy(ddq_bar + o, seed, n, cnt, cnt, in_ss, in_sj, stream));
    const int st = fwd_dyn_deriv_chunks(c, q + o, dq + o, tau + o, ddq_pass + o, q_bar ? Dq : nullptr, dq_bar ? Dv : nullptr, tau_bar ? Mi : nullptr,
                                        st_c, st_chunk, cnt, in_ss, in_sj, 1, cnt, chunk, image, comps, stream);
    if (st != RDYN_OK) return st;
    RdynVjpProductArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.dddq_dq = Dq;
    pa.dddq_dv = Dv;
    pa.minv = Mi;
    pa.ld = cnt;
    pa.n = n;
    pa.q = q + o;
    pa.dq = dq + o;
    pa.tau = tau + o;
    pa.ddq_bar = seed;
    pa.seed_ss = 1;
    pa.seed_sj = cnt;
    pa.q_bar = q_bar ? q_bar + o : nullptr;
    pa.dq_bar = dq_bar ? dq_bar + o : nullptr;
    pa.tau_bar = tau_bar ? tau_bar + o : nullptr;
    pa.ddq = ddq ? ddq + o : nullptr;
    pa.status = st_c;
    pa.n_samples = cnt;
    pa.in_ss = in_ss;
    pa.in_sj = in_sj;
    RDYN_HIP_TRY(rdyn_launch_vjp_products(pa, stream));
  }
  return RDYN_OK;
}

// ---- the entry points (C linkage from their declarations in include/rdyn.h) ------------------------------------------
size_t rdyn_forward_dynamics_workspace_bytes(const rdyn_chain* c, int64_t chunk_samples) { return fwd_layout(c, chunk_samples).total; }

int rdyn_forward_dynamics(const rdyn_chain* c, const rdyn_batch* b, const double* tau, double* ddq, int32_t* status, int64_t chunk_samples,
                          void* workspace, size_t workspace_bytes)
{
  return forward_dynamics(c, b, nullptr, 0, nullptr, tau, ddq, status, chunk_samples, workspace, workspace_bytes, "rdyn_forward_dynamics");
}

int rdyn_forward_dynamics_components(const rdyn_chain* c, const rdyn_batch* b, const rdyn_component* comps, int n_comps, const double* tau,
                                     double* ddq, int32_t* status, int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  return forward_dynamics(c, b, comps, n_comps, nullptr, tau, ddq, status, chunk_samples, workspace, workspace_bytes,
                          "rdyn_forward_dynamics_components");
}

size_t rdyn_forward_dynamics_ext_workspace_bytes(const rdyn_chain* c, const rdyn_ext_wrenches* ext, int64_t chunk_samples)
{
  return fwd_layout(c, chunk_samples, ext && ext->w).total;
}

int rdyn_forward_dynamics_ext(const rdyn_chain* c, const rdyn_batch* b, const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext,
                              const double* tau, double* ddq, int32_t* status, int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  return forward_dynamics(c, b, comps, n_comps, ext, tau, ddq, status, chunk_samples, workspace, workspace_bytes, "rdyn_forward_dynamics_ext");
}

size_t rdyn_rollout_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_desc* d, int64_t n_samples, int64_t chunk_samples)
{
  return rollout_layout(c, d, n_samples, chunk_samples).s.total;
}

int rdyn_rollout(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_desc* d, int64_t chunk_samples, void* workspace,
                 size_t workspace_bytes)
{
  return rollout(c, b, d, nullptr, 0, nullptr, chunk_samples, workspace, workspace_bytes, "rdyn_rollout");
}

int rdyn_rollout_components(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_desc* d, const rdyn_component* comps, int n_comps,
                            int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  return rollout(c, b, d, comps, n_comps, nullptr, chunk_samples, workspace, workspace_bytes, "rdyn_rollout_components");
}

size_t rdyn_rollout_ext_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_desc* d, const rdyn_ext_wrenches* ext, int64_t n_samples,
                                        int64_t chunk_samples)
{
  return rollout_layout(c, d, n_samples, chunk_samples, ext && ext->w).s.total;
}

size_t rdyn_rollout_feedback_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_desc* d, const rdyn_ext_wrenches* ext,
                                             const rdyn_feedback* fb, int64_t n_samples, int64_t chunk_samples)
{
  return rollout_layout(c, d, n_samples, chunk_samples, ext && ext->w, fb != nullptr).s.total;
}

int rdyn_rollout_feedback(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_desc* d, const rdyn_component* comps, int n_comps,
                          const rdyn_ext_wrenches* ext, const rdyn_feedback* fb, int64_t chunk_samples, void* workspace,
                          size_t workspace_bytes)
{
  return rollout(c, b, d, comps, n_comps, ext, chunk_samples, workspace, workspace_bytes, "rdyn_rollout_feedback", fb);
}

size_t rdyn_rollout_model_feedback_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_desc* d, const rdyn_ext_wrenches* ext,
                                                   const rdyn_feedback* fb, const rdyn_model_feedback* mfb, int64_t n_samples,
                                                   int64_t chunk_samples)
{
  return mfb ? 0 : rdyn_rollout_feedback_workspace_bytes(c, d, ext, fb, n_samples, chunk_samples);
}

int rdyn_rollout_model_feedback(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_desc* d, const rdyn_component* comps, int n_comps,
                                const rdyn_ext_wrenches* ext, const rdyn_feedback* fb, const rdyn_model_feedback* mfb, int64_t chunk_samples,
                                void* workspace, size_t workspace_bytes)
{
  if (!mfb) return rdyn_rollout_feedback(c, b, d, comps, n_comps, ext, fb, chunk_samples, workspace, workspace_bytes);
  return rollout(c, b, d, comps, n_comps, ext, chunk_samples, workspace, workspace_bytes, "rdyn_rollout_model_feedback", fb, mfb);
}

int rdyn_rollout_ext(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_desc* d, const rdyn_component* comps, int n_comps,
                     const rdyn_ext_wrenches* ext, int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  return rollout(c, b, d, comps, n_comps, ext, chunk_samples, workspace, workspace_bytes, "rdyn_rollout_ext");
}

size_t rdyn_forward_dynamics_derivatives_workspace_bytes(const rdyn_chain* c, int64_t chunk_samples)
{
  return deriv_layout(c, chunk_samples).total;
}

int rdyn_forward_dynamics_derivatives(const rdyn_chain* c, const rdyn_batch* b, const rdyn_component* comps, int n_comps, const double* tau,
                                      double* ddq, double* dddq_dq, double* dddq_dv, double* minv, int32_t* status, int64_t chunk_samples,
                                      void* workspace, size_t workspace_bytes)
{
  const char* const who = "rdyn_forward_dynamics_derivatives";
  int st = check_batch(c, b, true, false, who, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (b->n_samples > 0 && (!tau || !ddq)) return refuse(who, "null torque or acceleration pointer");
  if (b->n_samples > 0 && !dddq_dq && !dddq_dv && !minv) return refuse(who, "every matrix output is null");
  const DerivLayout L = deriv_layout(c, chunk_samples);
  DynCall k;
  st = dyn_prepare(c, b, comps, n_comps, chunk_samples, L.total, workspace, workspace_bytes, who, &k);
  if (st != RDYN_OK || !k.run) return st;
  int64_t m_ss, m_se;
  rec_strides(b, (int64_t)k.n * k.n, &m_ss, &m_se);
  if (k.sw)
  {
    RdynFwdDynDerivArgs a;
    memset(&a, 0, sizeof a);
    a.f.chain = k.chain;
    a.f.q = b->q;
    a.f.dq = b->dq;
    a.f.tau = tau;
    a.f.ddq = ddq;
    a.f.status = status;
    a.f.n_samples = b->n_samples;
    a.f.in_ss = k.in_ss;
    a.f.in_sj = k.in_sj;
    a.dddq_dq = dddq_dq;
    a.dddq_dv = dddq_dv;
    a.minv = minv;
    a.m_ss = m_ss;
    a.m_se = m_se;
    a.staged = stage_records(b, dddq_dq, dddq_dv, minv) ? k.n * k.n : 0;
    a.t = k.table;
    RDYN_HIP_TRY(rdyn_launch_forward_dynamics_derivatives(k.sw->n_joints(), a, k.stream));
    return RDYN_OK;
  }
  if ((dddq_dq || dddq_dv) && (st = long_deriv_lds_refusal(c, who)) != RDYN_OK) return st;
  return fwd_dyn_deriv_chunks(c, b->q, b->dq, tau, ddq, dddq_dq, dddq_dv, minv, status, (int32_t*)((char*)workspace + L.status), b->n_samples,
                              k.in_ss, k.in_sj, m_ss, m_se, L.f.chunk, (double*)workspace, k.comps, k.stream);
}

size_t rdyn_forward_dynamics_vjp_workspace_bytes(const rdyn_chain* c, int64_t chunk_samples) { return vjp_layout(c, chunk_samples).total; }

int rdyn_forward_dynamics_vjp(const rdyn_chain* c, const rdyn_batch* b, const rdyn_component* comps, int n_comps, const double* tau,
                              const double* ddq_bar, double* q_bar, double* dq_bar, double* tau_bar, double* ddq, int32_t* status,
                              int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  const char* const who = "rdyn_forward_dynamics_vjp";
  int st = check_batch(c, b, true, false, who, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (b->n_samples > 0 && (!tau || !ddq_bar)) return refuse(who, "null torque or seed pointer");
  if (b->n_samples > 0 && !q_bar && !dq_bar && !tau_bar) return refuse(who, "every product is null");
  const VjpLayout L = vjp_layout(c, chunk_samples);
  DynCall k;
  st = dyn_prepare(c, b, comps, n_comps, chunk_samples, L.total, workspace, workspace_bytes, who, &k);
  if (st != RDYN_OK || !k.run) return st;
  if (k.sw)
  {
    RdynFwdDynVjpArgs a;
    memset(&a, 0, sizeof a);
    a.chain = k.chain;
    a.q = b->q;
    a.dq = b->dq;
    a.tau = tau;
    a.ddq_bar = ddq_bar;
    a.q_bar = q_bar;
    a.dq_bar = dq_bar;
    a.tau_bar = tau_bar;
    a.ddq = ddq;
    a.status = status;
    a.n_samples = b->n_samples;
    a.in_ss = k.in_ss;
    a.in_sj = k.in_sj;
    a.staged = stage_records(b, q_bar, dq_bar, tau_bar, ddq) ? k.n : 0;
    a.t = k.table;
    RDYN_HIP_TRY(rdyn_launch_forward_dynamics_vjp(k.sw->n_joints(), a, k.stream));
    return RDYN_OK;
  }
  if ((q_bar || dq_bar) && (st = long_deriv_lds_refusal(c, who)) != RDYN_OK) return st;
  return vjp_chunks(c, b->q, b->dq, tau, ddq_bar, q_bar, dq_bar, tau_bar, ddq, status, b->n_samples, k.in_ss, k.in_sj, L, workspace, k.comps,
                    k.stream);
}

// ---- reverse-mode product with external link wrenches (rdyn_fwd_dyn_vjp_ext.hip) -------------------------------------
// Without wrenches the call IS rdyn_forward_dynamics_vjp.  With them: chains swept in registers, one launch, no workspace.
size_t rdyn_forward_dynamics_vjp_ext_workspace_bytes(const rdyn_chain* c, const rdyn_ext_wrenches* ext, int64_t chunk_samples)
{
  return (ext && ext->w) ? 0 : vjp_layout(c, chunk_samples).total;
}

int rdyn_forward_dynamics_vjp_ext(const rdyn_chain* c, const rdyn_batch* b, const rdyn_component* comps, int n_comps, const rdyn_ext_wrenches* ext,
                                  const double* tau, const double* ddq_bar, double* q_bar, double* dq_bar, double* tau_bar, double* ext_bar,
                                  double* ddq, int32_t* status, int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  const char* const who = "rdyn_forward_dynamics_vjp_ext";
  if (!ext || !ext->w)
  {
    if (ext_bar) return refuse(who, "ext_bar without external wrenches");
    return rdyn_forward_dynamics_vjp(c, b, comps, n_comps, tau, ddq_bar, q_bar, dq_bar, tau_bar, ddq, status, chunk_samples, workspace,
                                     workspace_bytes);
  }
  int st = check_batch(c, b, true, false, who, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (b->n_samples > 0 && (!tau || !ddq_bar)) return refuse(who, "null torque or seed pointer");
  if (b->n_samples > 0 && !q_bar && !dq_bar && !tau_bar && !ext_bar) return refuse(who, "every product is null");
  RdynExtArgs x;
  st = check_ext(c, b, ext, false, who, &x);
  if (st != RDYN_OK) return st;
  if ((st = ext_reverse_refusal(c, who)) != RDYN_OK) return st;
  DynCall k;
  st = dyn_prepare(c, b, comps, n_comps, chunk_samples, 0, workspace, workspace_bytes, who, &k);
  if (st != RDYN_OK || !k.run) return st;
  RdynFwdDynVjpExtArgs ax;
  memset(&ax, 0, sizeof ax);
  RdynFwdDynVjpArgs& a = ax.v;
  a.chain = k.chain;
  a.q = b->q;
  a.dq = b->dq;
  a.tau = tau;
  a.ddq_bar = ddq_bar;
  a.q_bar = q_bar;
  a.dq_bar = dq_bar;
  a.tau_bar = tau_bar;
  a.ddq = ddq;
  a.status = status;
  a.n_samples = b->n_samples;
  a.in_ss = k.in_ss;
  a.in_sj = k.in_sj;
  a.staged = stage_records(b, q_bar, dq_bar, tau_bar, ddq) ? k.n : 0;
  a.t = k.table;
  ax.x = x;
  ax.ext_bar = ext_bar;
  RDYN_HIP_TRY(rdyn_launch_forward_dynamics_vjp_ext(k.sw->n_joints(), ax, k.stream));
  return RDYN_OK;
}

// ---- reverse-mode product with respect to the parameters (rdyn_fwd_dyn_param_vjp.hip) ----------------------------
// Chains the unrolled kernels sweep (long ones through their reduced companion, the rows and sums expanded by X_f'): one launch, and two
// small ones behind it when a sum is asked for.  The workspace holds the waves' partial sums [ceil(N / 64)][10 n_swept + C] and their
// total [10 n_swept + C].
// More input joints: CORRECT, NOT FAST.  The chunked product of rdyn_forward_dynamics_vjp gives tau_bar, ddq and the status of the whole
// batch (into the caller's arrays, or arrays of the workspace); then per chunk the element-major image [Y | C] at that ddq -- the writer
// of the wide normal equations (ChunkImage) -- and k_param_rows_from_image; the sums are the fixed-order column sums of the ROWS (the
// caller's, or element-major rows in the workspace), so neither rows nor sums depend on chunk_samples.  Workspace: the product's | tau_bar
// | ddq (n N each) | status (N) | the image of one chunk | rows [P + C][N] | the totals [P + C].
namespace
{
struct ParamVjpLayout
{
  int cols;
  int64_t waves;
  size_t S, total;  // the partials at offset 0
  // the chunked route
  VjpLayout v;
  int64_t chunk;
  size_t tb, ddq, st, image, rows;
};
static ParamVjpLayout param_vjp_layout(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int64_t n_samples, int64_t chunk_samples)
{
  ParamVjpLayout L = {};
  if (!c || c->n_active() < 1 || n_samples <= 0 || chunk_samples < 0) return L;
  const int C = (comps && n_comps > 0 && n_comps <= RDYN_MAX_COMPONENTS) ? rdyn_components_columns(comps, n_comps) : 0;
  if (fwd_dyn_by_chunks(c))
  {
    const size_t n = (size_t)c->n_active(), N = (size_t)n_samples;
    L.cols = 10 * c->n_joints() + (C > 0 ? C : 0);
    L.v = vjp_layout(c, chunk_samples);
    L.chunk = wide_chunk(c, L.cols, chunk_samples);
    if (L.chunk > n_samples) L.chunk = (n_samples + 63) & ~(int64_t)63;
    L.tb = L.v.total;
    L.ddq = L.tb + align256(n * N * sizeof(double));
    L.st = L.ddq + align256(n * N * sizeof(double));
    L.image = L.st + align256(N * sizeof(int32_t));
    L.rows = L.image + align256((size_t)L.chunk * n * (L.cols + 1) * sizeof(double));
    L.S = L.rows + align256((size_t)L.cols * N * sizeof(double));
    L.total = L.S + align256((size_t)L.cols * sizeof(double));
    return L;
  }
  const rdyn_chain* const sw = c->long_chain() ? c->reduced.get() : c;
  L.cols = 10 * sw->n_joints() + (C > 0 ? C : 0);
  L.waves = (n_samples + 63) / 64;
  L.S = align256((size_t)L.waves * L.cols * sizeof(double));
  L.total = L.S + align256((size_t)L.cols * sizeof(double));
  return L;
}
}  // namespace

size_t rdyn_forward_dynamics_parameter_vjp_workspace_bytes(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int64_t n_samples,
                                                           int64_t chunk_samples)
{
  return param_vjp_layout(c, comps, n_comps, n_samples, chunk_samples).total;
}

int rdyn_forward_dynamics_parameter_vjp(const rdyn_chain* c, const rdyn_batch* b, const rdyn_component* comps, int n_comps, const double* tau,
                                        const double* ddq_bar, double* pi_bar, double* comp_bar, double* pi_bar_sum, double* comp_bar_sum,
                                        int accumulate, double* tau_bar, double* ddq, int32_t* status, int64_t chunk_samples, void* workspace,
                                        size_t workspace_bytes)
{
  const char* const who = "rdyn_forward_dynamics_parameter_vjp";
  int st = check_batch(c, b, true, false, who, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (b->n_samples > 0 && (!tau || !ddq_bar)) return refuse(who, "null torque or seed pointer");
  if (b->n_samples > 0 && !pi_bar && !comp_bar && !pi_bar_sum && !comp_bar_sum && !tau_bar) return refuse(who, "every product is null");
  if (accumulate != 0 && accumulate != 1) return refuse(who, "accumulate is 0 or 1");
  const bool sums = pi_bar_sum || comp_bar_sum;
  const ParamVjpLayout L = param_vjp_layout(c, comps, n_comps, b->n_samples, chunk_samples < 0 ? 0 : chunk_samples);
  DynCall k;
  st = dyn_prepare(c, b, comps, n_comps, chunk_samples, (sums || fwd_dyn_by_chunks(c)) ? L.total : 0, workspace, workspace_bytes, who, &k);
  if (st != RDYN_OK || !k.run) return st;
  const int C = n_comps > 0 ? rdyn_components_columns(comps, n_comps) : 0;
  if (!k.sw)
  {
    const int64_t N = b->n_samples;
    const int P = 10 * c->n_joints();
    char* const w = (char*)workspace;
    double* const tb = tau_bar ? tau_bar : (double*)(w + L.tb);
    double* const acc = ddq ? ddq : (double*)(w + L.ddq);
    int32_t* const stp = status ? status : (int32_t*)(w + L.st);
    st = vjp_chunks(c, b->q, b->dq, tau, ddq_bar, nullptr, nullptr, tb, acc, stp, N, k.in_ss, k.in_sj, L.v, workspace, k.comps, k.stream);
    if (st != RDYN_OK) return st;
    const bool want_pi = pi_bar || pi_bar_sum, want_comp = C > 0 && (comp_bar || comp_bar_sum);
    if (!want_pi && !want_comp) return RDYN_OK;
    // the rows: the caller's, or element-major ones in the workspace for the sums
    RdynParamProductArgs pa;
    memset(&pa, 0, sizeof pa);
    double* const ws_rows = (double*)(w + L.rows);
    double* pi_rows = pi_bar;
    double* comp_rows = comp_bar;
    rec_strides(b, P, &pa.pi_ss, &pa.pi_sc);
    rec_strides(b, C, &pa.comp_ss, &pa.comp_sc);
    if (!pi_rows && want_pi)
    {
      pi_rows = ws_rows;
      pa.pi_ss = 1;
      pa.pi_sc = N;
    }
    if (!comp_rows && want_comp)
    {
      comp_rows = ws_rows + (int64_t)P * N;
      pa.comp_ss = 1;
      pa.comp_sc = N;
    }
    RdynComponentArgs ca;
    memset(&ca, 0, sizeof ca);
    if (n_comps > 0 && (st = fill_components(comps, n_comps, k.n, &ca)) != RDYN_OK) return st;
    rdyn_batch bi = *b;
    bi.ddq = acc;
    double* const image = (double*)(w + L.image);
    ChunkImage img(c, &bi, nullptr, image, P + C, &ca, n_comps, C);
    st = img.bind(true);
    if (st != RDYN_OK) return st;
    const int64_t in_step = (b->layout == RDYN_LAYOUT_SAMPLE_MAJOR) ? k.n : 1;
    for (int64_t s0 = 0; s0 < N; s0 += L.chunk)
    {
      const int64_t cnt = (N - s0 < L.chunk) ? N - s0 : L.chunk;
      st = img.write(s0, cnt, 1, k.stream);
      if (st != RDYN_OK) return st;
      pa.image = image;
      pa.cnt = cnt;
      pa.lda = (int64_t)k.n * cnt;
      pa.n = k.n;
      pa.P = P;
      pa.K = C;
      pa.tau_bar = tb + s0 * in_step;
      pa.in_ss = k.in_ss;
      pa.in_sj = k.in_sj;
      pa.status = stp + s0;
      pa.pi_rows = pi_rows ? pi_rows + s0 * pa.pi_ss : nullptr;
      pa.comp_rows = comp_rows ? comp_rows + s0 * pa.comp_ss : nullptr;
      RDYN_HIP_TRY(rdyn_launch_parameter_rows_from_image(pa, k.stream));
    }
    if (!sums) return RDYN_OK;
    double* const S = (double*)(w + L.S);
    if (pi_bar_sum) RDYN_HIP_TRY(rdyn_launch_parameter_column_sums(pi_rows, N, pa.pi_ss, pa.pi_sc, stp, P, S, k.stream));
    if (comp_bar_sum && C > 0) RDYN_HIP_TRY(rdyn_launch_parameter_column_sums(comp_rows, N, pa.comp_ss, pa.comp_sc, stp, C, S + P, k.stream));
    RdynParamSumArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.S = S;
    fa.pi_sum = pi_bar_sum;
    fa.comp_sum = C > 0 ? comp_bar_sum : nullptr;
    fa.accumulate = accumulate;
    fa.n_swept = fa.n_full = c->n_joints();
    fa.n_comp_cols = C;
    RDYN_HIP_TRY(rdyn_launch_parameter_sums_finish(fa, k.stream));
    return RDYN_OK;
  }
  RdynFwdDynParamVjpArgs a;
  memset(&a, 0, sizeof a);
  a.v.chain = k.chain;
  a.v.q = b->q;
  a.v.dq = b->dq;
  a.v.tau = tau;
  a.v.ddq_bar = ddq_bar;
  a.v.tau_bar = tau_bar;
  a.v.ddq = ddq;
  a.v.status = status;
  a.v.n_samples = b->n_samples;
  a.v.in_ss = k.in_ss;
  a.v.in_sj = k.in_sj;
  a.v.staged = stage_records(b, tau_bar, ddq) ? k.n : 0;
  a.v.t = k.table;
  a.pi_bar = pi_bar;
  a.comp_bar = comp_bar;
  rec_strides(b, (int64_t)10 * c->n_joints(), &a.pi_ss, &a.pi_sc);
  rec_strides(b, C, &a.comp_ss, &a.comp_sc);
  a.partials = sums ? (double*)workspace : nullptr;
  a.n_comp_cols = C;
  RdynParamSumArgs sa;
  memset(&sa, 0, sizeof sa);
  a.n_full = sa.n_full = c->n_joints();
  if (k.sw != c)
  {
    st = device_expand(c, &a.expand);
    if (st != RDYN_OK) return st;
    sa.expand = a.expand;
    for (int f = 0; f < c->n_joints(); ++f) a.red_of[f] = sa.red_of[f] = c->red_of[f];
  }
  RDYN_HIP_TRY(rdyn_launch_forward_dynamics_parameter_vjp(k.sw->n_joints(), a, k.stream));
  if (!sums) return RDYN_OK;
  sa.S = (const double*)((char*)workspace + L.S);
  sa.pi_sum = pi_bar_sum;
  sa.comp_sum = comp_bar_sum;
  sa.accumulate = accumulate;
  sa.n_swept = k.sw->n_joints();
  sa.n_comp_cols = C;
  RDYN_HIP_TRY(rdyn_launch_parameter_sums(a.partials, L.waves, L.cols, 1, nullptr, sa, k.stream));
  return RDYN_OK;
}

// ---- adjoint of a rollout (rdyn_rollout_adjoint.hip) ------------------------------------------------------------
// Chains the unrolled kernels sweep: one launch for the whole horizon.  More input joints: a host loop over steps and stages on the state
// arrays of AdjointLayout, behind the workspace of the product.
size_t rdyn_rollout_adjoint_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_adjoint_desc* d, int64_t n_samples, int64_t chunk_samples)
{
  return adjoint_layout(c, d, n_samples, chunk_samples).s.total;
}

// With the parameter gradients (pg set; rdyn_rollout_adjoint_params.hip): the same launch with the PARAMS kernels, the lanes' accumulators
// [10 n_swept + C][N], the final statuses [N] and the column sums [10 n_swept + C] in the workspace, then the two launches of
// rdyn_launch_parameter_sums.  Chains the unrolled kernels do not sweep are refused.
namespace
{
struct AdjointParamLayout { int cols; size_t st, S, total; };  // the accumulators at offset 0
static AdjointParamLayout adjoint_param_layout(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int64_t n_samples)
{
  AdjointParamLayout L = {};
  if (!c || c->n_active() < 1 || n_samples <= 0 || fwd_dyn_by_chunks(c)) return L;
  const int C = (comps && n_comps > 0 && n_comps <= RDYN_MAX_COMPONENTS) ? rdyn_components_columns(comps, n_comps) : 0;
  const rdyn_chain* const sw = c->long_chain() ? c->reduced.get() : c;
  L.cols = 10 * sw->n_joints() + (C > 0 ? C : 0);
  L.st = align256((size_t)n_samples * L.cols * sizeof(double));
  L.S = L.st + align256((size_t)n_samples * sizeof(int32_t));
  L.total = L.S + align256((size_t)L.cols * sizeof(double));
  return L;
}

// who = the entry point (error texts); pg null: rdyn_rollout_adjoint; ext with w (never with pg): rdyn_rollout_adjoint_ext with wrenches,
// gext its gradient selection (may be null); fb: rdyn_rollout_adjoint_feedback with the law, gfb its gradient selection (may be null);
// fb with pg: rdyn_rollout_adjoint_feedback_parameters (rdyn_rollout_adjoint_fb_params.hip), the closed loop's launch with the
// accumulators of the parameter route and the same reduction behind it
static int rollout_adjoint(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_adjoint_desc* d, const rdyn_component* comps, int n_comps,
                           const rdyn_parameter_gradient* pg, bool with_pg, int64_t chunk_samples, void* workspace, size_t workspace_bytes,
                           const char* who, const rdyn_ext_wrenches* ext = nullptr, const rdyn_ext_wrench_gradient* gext = nullptr,
                           const rdyn_feedback* fb = nullptr, const rdyn_feedback_gradient* gfb = nullptr)
{
  int st = check_batch(c, b, true, false, who, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!d) return refuse(who, "null descriptor");
  if (with_pg && (!pg || (!pg->gpi && !pg->gcomp))) return refuse(who, "null parameter-gradient selection, or neither gpi nor gcomp in it");
  if (with_pg && pg->accumulate != 0 && pg->accumulate != 1) return refuse(who, "accumulate is 0 or 1");
  const int n = c->n_active();
  const int64_t N = b->n_samples;
  const int T = d->n_steps;
  st = check_integration(T, d->dt, d->integrator, d->tau, who);
  if (st != RDYN_OK) return st;
  if (T >= 2 && (!d->q_traj || !d->dq_traj))
    return refuse(who, "two or more steps need the forward call's trajectory (q_traj and dq_traj, traj_every = 1)");
  const int64_t nN = (int64_t)n * N;
  const bool running = d->gq_traj || d->gdq_traj;
  if ((T >= 2 && d->traj_step_stride < nN) || (running && d->gtraj_step_stride < nN) ||
      (d->gtau && d->gtau_step_stride != 0 && d->gtau_step_stride < nN))
    return refuse(who, "traj_step_stride, gtraj_step_stride and a non-zero gtau_step_stride must be >= n * n_samples");
  RdynExtArgs x;
  st = check_ext(c, b, ext, true, who, &x);
  if (st != RDYN_OK) return st;
  double* const gw = (x.w && gext) ? gext->gw : nullptr;
  if (gw)
  {
    const int64_t rec = (x.one ? 6 : 6 * (int64_t)(c->n_joints() + 1)) * N;
    if (gext->step_stride < 0 || (gext->step_stride != 0 && gext->step_stride < rec))
    {
      rdyn_set_error("%s: wrench-gradient step_stride %lld is negative, or not zero and smaller than one step's record (%lld doubles)", who,
                     (long long)gext->step_stride, (long long)rec);
      return RDYN_ERR_INVALID_ARGUMENT;
    }
  }
  RdynFeedbackGradArgs gf;
  memset(&gf, 0, sizeof gf);
  if (fb)
  {
    if (!fb->q_ref || !fb->kp) return refuse(who, "null reference (q_ref) or gain (kp) pointer");
    if (fb->ref_step_stride < 0 || (fb->ref_step_stride != 0 && fb->ref_step_stride < nN))
    {
      rdyn_set_error("%s: ref_step_stride %lld is negative, or not zero and smaller than one step's record (%lld doubles)", who,
                     (long long)fb->ref_step_stride, (long long)nN);
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    if ((fb->hold != 0 && fb->hold != 1) || (fb->gains_per_sample != 0 && fb->gains_per_sample != 1))
      return refuse(who, "hold and gains_per_sample are 0 or 1");
    if (gfb)
    {
      if ((gfb->gkd || gfb->gdq_ref) && !fb->kd) return refuse(who, "gkd or gdq_ref without a velocity gain (fb->kd)");
      if (gfb->glim && !fb->tau_limit) return refuse(who, "glim without limits (fb->tau_limit)");
      if ((gfb->gq_ref || gfb->gdq_ref) && (gfb->gref_step_stride < 0 || (gfb->gref_step_stride != 0 && gfb->gref_step_stride < nN)))
      {
        rdyn_set_error("%s: gref_step_stride %lld is negative, or not zero and smaller than one step's record (%lld doubles)", who,
                       (long long)gfb->gref_step_stride, (long long)nN);
        return RDYN_ERR_INVALID_ARGUMENT;
      }
      if (gfb->gu_traj && gfb->gu_step_stride < nN) return refuse(who, "gu_traj needs gu_step_stride >= n * n_samples");
      if (gfb->accumulate != 0 && gfb->accumulate != 1) return refuse(who, "accumulate is 0 or 1");
      gf.gq_ref = gfb->gq_ref;
      gf.gdq_ref = gfb->gdq_ref;
      gf.gref_step = (gfb->gq_ref || gfb->gdq_ref) ? gfb->gref_step_stride : 0;
      gf.gkp = gfb->gkp;
      gf.gkd = gfb->gkd;
      gf.glim = gfb->glim;
      gf.gu = gfb->gu_traj;
      gf.gu_step = gfb->gu_traj ? gfb->gu_step_stride : 0;
      gf.accumulate = gfb->accumulate;
    }
  }
  const bool law_out = gf.gq_ref || gf.gdq_ref || gf.gkp || gf.gkd || gf.glim;
  if (N > 0 && !with_pg && !d->gq0 && !d->gdq0 && !d->gtau && !gw && !law_out) return refuse(who, "every output is null");
  if (x.w && with_pg)
  {
    rdyn_set_error("%s: the parameter gradients with external wrenches are the follow-up: rdyn_rollout_adjoint_feedback serves the wrenches, "
                   "this call the parameters, not yet both",
                   who);
    return RDYN_ERR_UNSUPPORTED;
  }
  if (x.w && (st = ext_reverse_refusal(c, who)) != RDYN_OK) return st;
  if (fb && fwd_dyn_by_chunks(c))
  {
    rdyn_set_error("%s: chains that rdyn_rollout_feedback serves by its chunked route (more than %d input joints; this chain has %d) are not "
                   "served yet: the adjoint of the chunked closed loop is the follow-up",
                   who, RDYN_MAX_SWEPT_JOINTS, n);
    return RDYN_ERR_UNSUPPORTED;
  }
  if (with_pg && fwd_dyn_by_chunks(c))
  {
    rdyn_set_error("%s: chains with more than %d input joints are not served yet (this chain has %d); rdyn_rollout_adjoint serves them", who,
                   RDYN_MAX_SWEPT_JOINTS, n);
    return RDYN_ERR_UNSUPPORTED;
  }
  const AdjointLayout L = adjoint_layout(c, d, N, chunk_samples);
  const AdjointParamLayout PL = adjoint_param_layout(c, comps, n_comps, with_pg ? N : 0);
  DynCall k;
  st = dyn_prepare(c, b, comps, n_comps, chunk_samples, with_pg ? PL.total : ((x.w || fb) ? 0 : L.s.total), workspace, workspace_bytes, who, &k);
  if (st != RDYN_OK || !k.run) return st;
  if (k.sw)
  {
    RdynRolloutAdjointArgs a;
    memset(&a, 0, sizeof a);
    a.chain = k.chain;
    a.q = b->q;
    a.dq = b->dq;
    a.tau = d->tau;
    a.tau_step = d->tau_step_stride;
    a.q_traj = d->q_traj;
    a.dq_traj = d->dq_traj;
    a.traj_step = d->traj_step_stride;
    a.gq_end = d->gq_end;
    a.gdq_end = d->gdq_end;
    a.gq_traj = d->gq_traj;
    a.gdq_traj = d->gdq_traj;
    a.gtraj_step = d->gtraj_step_stride;
    a.gq0 = d->gq0;
    a.gdq0 = d->gdq0;
    a.gtau = d->gtau;
    a.gtau_step = d->gtau_step_stride;
    a.status = d->status;
    a.n_samples = N;
    a.in_ss = k.in_ss;
    a.in_sj = k.in_sj;
    a.dt = d->dt;
    a.n_steps = T;
    a.integrator = d->integrator;
    a.n_active = n;
    // whole lines: every record of the kind starts on a line (the step stride keeps the alignment of the first record)
    if ((d->gq0 || d->gdq0) && stage_records(b, d->gq0, d->gdq0)) a.staged |= 1;
    if (d->gtau && stage_records(b, d->gtau) && (d->gtau_step_stride * (int64_t)sizeof(double)) % 128 == 0) a.staged |= 2;
    a.t = k.table;
    RdynRolloutAdjointFbArgs af;
    memset(&af, 0, sizeof af);
    if (fb)
    {
      af.ax.a = a;
      af.ax.x = x;
      af.ax.gw = gw;
      af.ax.gw_step = gw ? gext->step_stride : 0;
      af.f.q_ref = fb->q_ref;
      af.f.dq_ref = fb->dq_ref;
      af.f.ref_step = fb->ref_step_stride;
      af.f.kp = fb->kp;
      af.f.kd = fb->kd;
      af.f.lim = fb->tau_limit;
      af.f.per_sample = fb->gains_per_sample;
      af.f.hold = fb->hold;
      af.g = gf;
      if ((gf.gq_ref || gf.gdq_ref) && gf.gref_step != 0 && stage_records(b, gf.gq_ref, gf.gdq_ref) &&
          (gf.gref_step * (int64_t)sizeof(double)) % 128 == 0)
        af.g.staged = 1;
      if (!with_pg)
      {
        RDYN_HIP_TRY(rdyn_launch_rollout_adjoint_feedback(k.sw->n_joints(), af, k.stream));
        return RDYN_OK;
      }
    }
    if (x.w && !fb)
    {
      RdynRolloutAdjointExtArgs ax;
      memset(&ax, 0, sizeof ax);
      ax.a = a;
      ax.x = x;
      ax.gw = gw;
      ax.gw_step = gw ? gext->step_stride : 0;
      if (d->integrator == RDYN_INTEGRATOR_RK4)
        RDYN_HIP_TRY(rdyn_launch_rollout_adjoint_ext_rk4(k.sw->n_joints(), ax, k.stream));
      else
        RDYN_HIP_TRY(rdyn_launch_rollout_adjoint_ext_euler(k.sw->n_joints(), ax, k.stream));
      return RDYN_OK;
    }
    if (!with_pg)
    {
      RDYN_HIP_TRY(rdyn_launch_rollout_adjoint(k.sw->n_joints(), a, k.stream));
      return RDYN_OK;
    }
    const int C = n_comps > 0 ? rdyn_components_columns(comps, n_comps) : 0;
    double* const acc = (double*)workspace;
    int32_t* const st_final = (int32_t*)((char*)workspace + PL.st);
    RdynParamSumArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.n_full = c->n_joints();
    if (k.sw != c)
    {
      st = device_expand(c, &sa.expand);
      if (st != RDYN_OK) return st;
      for (int f = 0; f < c->n_joints(); ++f) sa.red_of[f] = c->red_of[f];
    }
    const bool rk4 = d->integrator == RDYN_INTEGRATOR_RK4;
    if (fb && rk4)
      RDYN_HIP_TRY(rdyn_launch_rollout_adjoint_feedback_params_rk4(k.sw->n_joints(), af, acc, N, st_final, C, k.stream));
    else if (fb)
      RDYN_HIP_TRY(rdyn_launch_rollout_adjoint_feedback_params_euler(k.sw->n_joints(), af, acc, N, st_final, C, k.stream));
    else if (rk4)
      RDYN_HIP_TRY(rdyn_launch_rollout_adjoint_params_rk4(k.sw->n_joints(), a, acc, N, st_final, C, k.stream));
    else
      RDYN_HIP_TRY(rdyn_launch_rollout_adjoint_params_euler(k.sw->n_joints(), a, acc, N, st_final, C, k.stream));
    sa.S = (const double*)((char*)workspace + PL.S);
    sa.pi_sum = pg->gpi;
    sa.comp_sum = pg->gcomp;
    sa.accumulate = pg->accumulate;
    sa.n_swept = k.sw->n_joints();
    sa.n_comp_cols = C;
    RDYN_HIP_TRY(rdyn_launch_parameter_sums(acc, N, 1, N, st_final, sa, k.stream));
    return RDYN_OK;
  }
  if (T > 0 && (st = long_deriv_lds_refusal(c, who)) != RDYN_OK) return st;
  const int64_t in_ss = k.in_ss, in_sj = k.in_sj;
  hipStream_t stream = k.stream;
  double* ws[18];
  for (size_t i = 0; i < 18; ++i) ws[i] = L.s.array(workspace, i);
  int32_t* const st_stage = (int32_t*)((char*)workspace + L.s.st_stage);
  int32_t* const st_run = (int32_t*)((char*)workspace + L.s.st_run);
  double *const lq = ws[0], *const lv = ws[1], *const mu = ws[2], *const qb = ws[3], *const vb = ws[4], *const tb = ws[5];
  double* const acc = ws[17];
  RdynAdjointUpdateArgs u;
  memset(&u, 0, sizeof u);
  u.lq = lq;
  u.lv = lv;
  u.mv = mu;
  u.qb = qb;
  u.vb = vb;
  u.tb = tb;
  u.xq = ws[6];
  u.xv = ws[7];
  u.kq = ws[8];
  u.kv = ws[9];
  u.mq = ws[10];
  u.st_stage = st_stage;
  u.st_run = st_run;
  u.count = nN;
  u.n_samples = N;
  u.n = n;
  u.element_major = b->layout == RDYN_LAYOUT_ELEMENT_MAJOR;
  u.dt = d->dt;
  const bool gsum = d->gtau && d->gtau_step_stride == 0;
  auto update = [&](int op) -> hipError_t {
    u.op = op;
    return rdyn_launch_adjoint_update(u, stream);
  };
  const int64_t last = (int64_t)(T - 1) * d->gtraj_step_stride;
  u.a = d->gq_end;
  u.b = (T > 0 && d->gq_traj) ? d->gq_traj + last : nullptr;
  u.c = d->gdq_end;
  u.d = (T > 0 && d->gdq_traj) ? d->gdq_traj + last : nullptr;
  RDYN_HIP_TRY(update(RDYN_ADJ_OP_INIT));
  if (gsum)
  {
    u.gtau = d->gtau;
    RDYN_HIP_TRY(update(RDYN_ADJ_OP_ZERO));
  }
  for (int t = T - 1; t >= 0; --t)
  {
    const double* const xq_t = t == 0 ? b->q : d->q_traj + (int64_t)(t - 1) * d->traj_step_stride;
    const double* const xv_t = t == 0 ? b->dq : d->dq_traj + (int64_t)(t - 1) * d->traj_step_stride;
    const double* const tau_t = d->tau + (int64_t)t * d->tau_step_stride;
    u.gtau = d->gtau ? d->gtau + (int64_t)t * d->gtau_step_stride : nullptr;
    u.gtau_add = gsum;
    if (d->integrator == RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER)
    {
      RDYN_HIP_TRY(update(RDYN_ADJ_OP_EULER_PRE));
      st = vjp_chunks(c, xq_t, xv_t, tau_t, mu, qb, vb, tb, nullptr, st_stage, N, in_ss, in_sj, L.v, workspace, k.comps, stream);
      if (st != RDYN_OK) return st;
      RDYN_HIP_TRY(update(RDYN_ADJ_OP_EULER_POST));
    }
    else
    {
      // the stage states X2 .. X4 (X1 = x_t): ws[11 + 2 (i - 2)], ws[12 + 2 (i - 2)]
      for (int stage = 0; stage < 3; ++stage)
      {
        const double* const sq = stage ? ws[11 + 2 * (stage - 1)] : xq_t;
        const double* const sv = stage ? ws[12 + 2 * (stage - 1)] : xv_t;
        st = fwd_dyn_chunks(c, sq, sv, tau_t, acc, st_stage, N, in_ss, in_sj, L.v.d.f.chunk, (double*)workspace, stream, k.comps);
        if (st != RDYN_OK) return st;
        u.a = xq_t;
        u.b = xv_t;
        u.c = sv;
        u.d = acc;
        u.sq = ws[11 + 2 * stage];
        u.sv = ws[12 + 2 * stage];
        u.cdt = stage == 2 ? d->dt : 0.5 * d->dt;  // of the NEXT stage
        RDYN_HIP_TRY(update(RDYN_ADJ_OP_RK4_FWD));
      }
      RDYN_HIP_TRY(update(RDYN_ADJ_OP_RK4_PRE));
      for (int i = 3; i >= 0; --i)
      {
        u.wgt = (i == 0 || i == 3) ? 1.0 / 6.0 : 1.0 / 3.0;
        u.cdt = i == 3 ? d->dt : 0.5 * d->dt;
        RDYN_HIP_TRY(update(RDYN_ADJ_OP_RK4_SEED));
        st = vjp_chunks(c, i ? ws[11 + 2 * (i - 1)] : xq_t, i ? ws[12 + 2 * (i - 1)] : xv_t, tau_t, mu, qb, vb, tb, nullptr, st_stage, N, in_ss,
                        in_sj, L.v, workspace, k.comps, stream);
        if (st != RDYN_OK) return st;
        RDYN_HIP_TRY(update(RDYN_ADJ_OP_RK4_POST));
      }
      RDYN_HIP_TRY(update(RDYN_ADJ_OP_RK4_END));
    }
    if (t >= 1 && running)
    {
      u.a = d->gq_traj ? d->gq_traj + (int64_t)(t - 1) * d->gtraj_step_stride : nullptr;
      u.b = d->gdq_traj ? d->gdq_traj + (int64_t)(t - 1) * d->gtraj_step_stride : nullptr;
      RDYN_HIP_TRY(update(RDYN_ADJ_OP_ADD_SEED));
    }
  }
  u.out_q = d->gq0;
  u.out_v = d->gdq0;
  u.status = d->status;
  RDYN_HIP_TRY(update(RDYN_ADJ_OP_OUT));
  return RDYN_OK;
}
}  // namespace

int rdyn_rollout_adjoint(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_adjoint_desc* d, const rdyn_component* comps, int n_comps,
                         int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  return rollout_adjoint(c, b, d, comps, n_comps, nullptr, false, chunk_samples, workspace, workspace_bytes, "rdyn_rollout_adjoint");
}

size_t rdyn_rollout_adjoint_parameters_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_adjoint_desc* d, const rdyn_component* comps,
                                                       int n_comps, int64_t n_samples, int64_t chunk_samples)
{
  return (!d || chunk_samples < 0) ? 0 : adjoint_param_layout(c, comps, n_comps, n_samples).total;
}

int rdyn_rollout_adjoint_parameters(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_adjoint_desc* d, const rdyn_component* comps,
                                    int n_comps, const rdyn_parameter_gradient* pg, int64_t chunk_samples, void* workspace,
                                    size_t workspace_bytes)
{
  return rollout_adjoint(c, b, d, comps, n_comps, pg, true, chunk_samples, workspace, workspace_bytes, "rdyn_rollout_adjoint_parameters");
}

size_t rdyn_rollout_adjoint_ext_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_adjoint_desc* d, const rdyn_ext_wrenches* ext,
                                                int64_t n_samples, int64_t chunk_samples)
{
  return (ext && ext->w) ? 0 : adjoint_layout(c, d, n_samples, chunk_samples).s.total;
}

int rdyn_rollout_adjoint_ext(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_adjoint_desc* d, const rdyn_component* comps, int n_comps,
                             const rdyn_ext_wrenches* ext, const rdyn_ext_wrench_gradient* gext, int64_t chunk_samples, void* workspace,
                             size_t workspace_bytes)
{
  const char* const who = "rdyn_rollout_adjoint_ext";
  if (!ext || !ext->w)
  {
    if (gext && gext->gw) return refuse(who, "a wrench gradient without external wrenches");
    return rollout_adjoint(c, b, d, comps, n_comps, nullptr, false, chunk_samples, workspace, workspace_bytes, "rdyn_rollout_adjoint");
  }
  return rollout_adjoint(c, b, d, comps, n_comps, nullptr, false, chunk_samples, workspace, workspace_bytes, who, ext, gext);
}

size_t rdyn_rollout_adjoint_feedback_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_adjoint_desc* d, const rdyn_ext_wrenches* ext,
                                                     const rdyn_feedback* fb, int64_t n_samples, int64_t chunk_samples)
{
  return fb ? 0 : rdyn_rollout_adjoint_ext_workspace_bytes(c, d, ext, n_samples, chunk_samples);
}

int rdyn_rollout_adjoint_feedback(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_adjoint_desc* d, const rdyn_component* comps,
                                  int n_comps, const rdyn_ext_wrenches* ext, const rdyn_ext_wrench_gradient* gext, const rdyn_feedback* fb,
                                  const rdyn_feedback_gradient* gfb, int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  const char* const who = "rdyn_rollout_adjoint_feedback";
  if (!fb)
  {
    if (gfb && (gfb->gq_ref || gfb->gdq_ref || gfb->gkp || gfb->gkd || gfb->glim || gfb->gu_traj))
      return refuse(who, "a feedback gradient without a feedback law");
    return rdyn_rollout_adjoint_ext(c, b, d, comps, n_comps, ext, gext, chunk_samples, workspace, workspace_bytes);
  }
  if ((!ext || !ext->w) && gext && gext->gw) return refuse(who, "a wrench gradient without external wrenches");
  return rollout_adjoint(c, b, d, comps, n_comps, nullptr, false, chunk_samples, workspace, workspace_bytes, who, ext, gext, fb, gfb);
}

size_t rdyn_rollout_adjoint_feedback_parameters_workspace_bytes(const rdyn_chain* c, const rdyn_rollout_adjoint_desc* d, const rdyn_component* comps,
                                                                int n_comps, const rdyn_ext_wrenches* ext, const rdyn_feedback* fb,
                                                                int64_t n_samples, int64_t chunk_samples)
{
  (void)fb;  // the law needs no workspace: with it or without, the accumulators of the parameter route
  if (ext && ext->w) return 0;  // refused
  return rdyn_rollout_adjoint_parameters_workspace_bytes(c, d, comps, n_comps, n_samples, chunk_samples);
}

int rdyn_rollout_adjoint_feedback_parameters(const rdyn_chain* c, const rdyn_batch* b, const rdyn_rollout_adjoint_desc* d, const rdyn_component* comps,
                                             int n_comps, const rdyn_ext_wrenches* ext, const rdyn_ext_wrench_gradient* gext,
                                             const rdyn_feedback* fb, const rdyn_feedback_gradient* gfb, const rdyn_parameter_gradient* pg,
                                             int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  const char* const who = "rdyn_rollout_adjoint_feedback_parameters";
  if (!fb && gfb && (gfb->gq_ref || gfb->gdq_ref || gfb->gkp || gfb->gkd || gfb->glim || gfb->gu_traj))
    return refuse(who, "a feedback gradient without a feedback law");
  if ((!ext || !ext->w) && gext && gext->gw) return refuse(who, "a wrench gradient without external wrenches");
  if (!fb && (!ext || !ext->w)) return rdyn_rollout_adjoint_parameters(c, b, d, comps, n_comps, pg, chunk_samples, workspace, workspace_bytes);
  return rollout_adjoint(c, b, d, comps, n_comps, pg, true, chunk_samples, workspace, workspace_bytes, who, ext, gext, fb, gfb);
}
