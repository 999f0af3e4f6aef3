// rdyn_api.cpp -- batched C-ABI entry points (include/rdyn.h): argument checks, layout -> strides,
// chain-constant residency per device, kernel launches.  No host<->device copies of batch data, no
// allocation and no synchronisation after a chain's first use on a device.
// This file: residency and the batch checks, regressor / torque / inertia and the torque derivatives, the base and ext sweeps, IK and
// frame distance, components, the mixed-chain plan, rdyn_evaluate_all.  The forward-dynamics family is rdyn_api_dynamics.cpp, the
// normal equations rdyn_api_gram.cpp, the R factors rdyn_api_tsqr.cpp; what they share (and the list of the diagnostic environment
// switches) is rdyn_api_common.h.
#include <map>
#include <memory>
#include <vector>

#include "rdyn_api_common.h"

int device_const(const rdyn_chain* c, const RdynChainConst** out)
{
  if (c->long_chain())
  {
    rdyn_set_error("chains of more than %d joints are served through their reduced companion only", RDYN_MAX_SWEPT_JOINTS);
    return RDYN_ERR_UNSUPPORTED;
  }
  int dev = 0;
  RDYN_HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(c->mu);
  auto it = c->dev_const.find(dev);
  if (it == c->dev_const.end())
  {
    RdynChainConst* d = nullptr;
    RDYN_HIP_TRY(hipMalloc((void**)&d, sizeof(RdynChainConst)));
    hipError_t e = hipMemcpy(d, &c->host_const, sizeof(RdynChainConst), hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
      (void)hipFree(d);
      rdyn_set_error("HIP error: %s (upload of chain constants)", hipGetErrorString(e));
      return RDYN_ERR_HIP;
    }
    it = c->dev_const.emplace(dev, d).first;
  }
  *out = it->second;
  return RDYN_OK;
}

// constants of a chain of more than RDYN_MAX_SWEPT_JOINTS joints for the run-time-length kinematic kernels (rdyn_long_kin.hip)
int device_const_long(const rdyn_chain* c, const RdynLongChainConst** out)
{
  int dev = 0;
  RDYN_HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(c->mu);
  auto it = c->dev_long.find(dev);
  if (it == c->dev_long.end())
  {
    RdynLongChainConst* d = nullptr;
    RDYN_HIP_TRY(hipMalloc((void**)&d, sizeof(RdynLongChainConst)));
    hipError_t e = hipMemcpy(d, &c->host_long, sizeof(RdynLongChainConst), hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
      (void)hipFree(d);
      rdyn_set_error("HIP error: %s (upload of chain constants)", hipGetErrorString(e));
      return RDYN_ERR_HIP;
    }
    it = c->dev_long.emplace(dev, d).first;
  }
  *out = it->second;
  return RDYN_OK;
}

// device copy of the expansion blocks X_f of a chain with a reduced companion (rdyn_chain.hpp), current device
int device_expand(const rdyn_chain* c, const double** out)
{
  int dev = 0;
  RDYN_HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(c->mu);
  auto it = c->dev_expand.find(dev);
  if (it == c->dev_expand.end())
  {
    double* d = nullptr;
    const size_t bytes = c->expand_X.size() * sizeof(double);
    RDYN_HIP_TRY(hipMalloc((void**)&d, bytes));
    hipError_t e = hipMemcpy(d, c->expand_X.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
      (void)hipFree(d);
      rdyn_set_error("HIP error: %s (upload of the expansion blocks)", hipGetErrorString(e));
      return RDYN_ERR_HIP;
    }
    it = c->dev_expand.emplace(dev, d).first;
  }
  *out = it->second;
  return RDYN_OK;
}

int check_batch(const rdyn_chain* c, const rdyn_batch* b, bool need_dq, bool need_ddq, const char* fn, int long_mode)
{
  if (!c || !b)
  {
    rdyn_set_error("%s: null chain or batch", fn);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (c->long_chain() && long_mode == LONG_NONE)
  {
    rdyn_set_error("%s: chains of more than %d joints are not served by this entry point", fn, RDYN_MAX_SWEPT_JOINTS);
    return RDYN_ERR_UNSUPPORTED;
  }
  if (c->long_chain() && long_mode == LONG_COMPANION && !c->reduced)
  {
    rdyn_set_error("%s: a chain of %d joints needs at most %d input joints", fn, c->n_joints(), RDYN_MAX_SWEPT_JOINTS);
    return RDYN_ERR_UNSUPPORTED;
  }
  if (b->n_samples < 0 || (b->layout != RDYN_LAYOUT_SAMPLE_MAJOR && b->layout != RDYN_LAYOUT_ELEMENT_MAJOR))
  {
    rdyn_set_error("%s: invalid n_samples or layout", fn);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (c->n_joints() < 1)
  {
    rdyn_set_error("%s: chain has no joints", fn);
    return RDYN_ERR_UNSUPPORTED;
  }
  if (b->n_samples > 0 && (!b->q || (need_dq && !b->dq) || (need_ddq && !b->ddq)))
  {
    // the reference checks only getRegressor's dimensions (primitives_impl.h:1299-1309)
    rdyn_set_error("Input data dimensions mismatch");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  return RDYN_OK;
}

int fill_components(const rdyn_component* comps, int n_comps, int n_active, RdynComponentArgs* a)
{
  for (int i = 0; i < n_comps; ++i)
  {
    const rdyn_component& c = comps[i];
    if (c.type < RDYN_COMP_FRICTION1 || c.type > RDYN_COMP_SPRING || c.joint < 0 || c.joint >= n_active)
    {
      rdyn_set_error("component %d has an invalid type or joint", i);
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    a->comps[i].type = c.type;
    a->comps[i].joint = c.joint;
    a->comps[i].min_velocity = c.min_velocity < 1e-6 ? 1e-6 : c.min_velocity;  // friction_polynomial1.h:73-78
    a->comps[i].max_velocity = c.max_velocity <= 0 ? 1.0e6 : c.max_velocity;   // friction_polynomial1.h:81-86
    for (int k = 0; k < 3; ++k) a->comps[i].parameters[k] = c.parameters[k];
  }
  return RDYN_OK;
}

namespace
{

// Which row-contiguous regressor kernel (rdyn_image.hip) serves this layout: 0 none, 1 the per-sample image (stride_row 1, stride_col n,
// stride_sample >= n P), 2 the stacked (N n) x P matrix (stride_sample == n).  Needs the input joints in chain order and a compiled
// fixed-joint pattern (*fix_mask: bit f = chain joint f is not an input joint), and a 16-byte aligned Y: the copy-out moves 16-byte
// chunks whose addresses are Y + a multiple of 16 (an 8-byte aligned base -- a view at an odd double offset -- would put the last
// chunk of every image 8 bytes past its end); such calls keep the row-pair / strided kernels.
int image_route(const rdyn_chain* c, const rdyn_regressor_layout* yl, int64_t n_samples, const double* Y, bool multi, unsigned* fix_mask, bool* mapped = nullptr)
{
  if (mapped) *mapped = false;
  const int n = c->n_active(), nJ = c->n_joints();
  const bool lay_image = yl->stride_row == 1 && yl->stride_col == n && yl->stride_sample >= (int64_t)n * 10 * nJ;
  const bool lay_stacked = yl->stride_row == 1 && yl->stride_sample == n && yl->stride_col >= n_samples * n;
  if (!(lay_image || lay_stacked)) return 0;
  // less than one wave of samples (the facade's single-sample getRegressor): the staging machinery costs more than it saves (19.5 us per
  // call at N = 1 against 11 for the kernels that store from the computing lane, profiles/r6/perf_sheet.txt) -- the row-pair / strided kernels
  if (n_samples < 64 && !multi) return 0;
  if (((uintptr_t)Y & 15u) != 0) return 0;
  if (lay_stacked && (yl->stride_col * 8) % 16 != 0) return 0;  // every column must start 16-byte aligned too
  unsigned fix = (nJ >= 32) ? 0u : ((1u << nJ) - 1u);
  bool ordered_inputs = true;
  for (int j = 0; j < n; ++j)
  {
    if (j > 0 && c->active[j] <= c->active[j - 1]) ordered_inputs = false;
    fix &= ~(1u << c->active[j]);
  }
  *fix_mask = fix;
  if (ordered_inputs && rdyn_image_supported(nJ, fix, yl->stride_sample, multi)) return lay_stacked ? 2 : 1;
  // input joints out of chain order, or joints that are not input joints somewhere else than the compiled head / tail patterns:
  // per-sample images go through the run-time row map (k_image_sweep<.., MAP>); everything else keeps the row-pair / strided kernels
  if (mapped && !multi && lay_image && !lay_stacked && (ordered_inputs || c->sorted) && rdyn_image_map_supported(nJ, fix, yl->stride_sample))
  {
    *mapped = true;
    return 1;
  }
  return 0;
}

int run_local(const rdyn_chain* c, const rdyn_batch* b, int mode, double* tau, double* Y, const rdyn_regressor_layout* yl, double* M,
              bool use_dq, bool use_ddq)
{
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  int st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  RdynSweepArgs a;
  memset(&a, 0, sizeof a);
  // a chain longer than the kernels sweep: its reduced companion has the same input joints, torques and joint-space inertia; the
  // dense regressor is the companion's with every body's ten-vector multiplied by the blocks of the links that ride on it
  const rdyn_chain* const full = c;
  if (c->long_chain())
  {
    if (mode == RDYN_MODE_REGRESSOR)
    {
      mode = RDYN_MODE_REGRESSOR_EXPAND;
      st = device_expand(full, &a.expand_X);
      if (st != RDYN_OK) return st;
      a.expand_n = full->n_joints();
      for (int f = 0; f < full->n_joints(); ++f) a.expand_red_of[f] = full->red_of[f];
    }
    c = full->reduced.get();
  }
  st = device_const(c, &a.chain);
  if (st != RDYN_OK) return st;
  const int n = c->n_active();
  a.q = b->q;
  a.dq = use_dq ? b->dq : nullptr;
  a.ddq = use_ddq ? b->ddq : nullptr;
  a.n_samples = b->n_samples;
  rec_strides(b, n, &a.in_ss, &a.in_sj);
  a.tau = tau;
  a.tau_ss = a.in_ss;
  a.tau_sj = a.in_sj;
  a.Y = Y;
  if (yl)
  {
    a.y_ss = yl->stride_sample;
    a.y_sr = yl->stride_row;
    a.y_sc = yl->stride_col;
  }
  if (mode == RDYN_MODE_REGRESSOR_EXPAND && yl && yl->stride_row == 1 && ((uintptr_t)Y & 15) == 0)
  {
    // row-contiguous layouts: every link's block through the wave's LDS tile, copied out 16 bytes per lane (k_expand_staged)
    if (yl->stride_col == n && yl->stride_sample % 2 == 0) a.expand_stage = 1;        // per-sample images
    else if (yl->stride_sample == n && yl->stride_col % 2 == 0) a.expand_stage = 2;   // stacked (N n) x P matrix
    if (a.expand_stage) mode = RDYN_MODE_REGRESSOR_EXPAND_STAGED;
  }
  // per-sample images of a long chain whose companion has up to 6 joints: the image kernel (whole-line copy-out through the per-sample
  // ring) forms the blocks of the riding links one at a time (k_image_sweep<.., EXPAND>)
  bool expand_image = false;
  if (mode == RDYN_MODE_REGRESSOR_EXPAND_STAGED && a.expand_stage == 1 && c->n_active() == c->n_joints() &&
      rdyn_image_expand_supported(c->n_joints(), full->n_joints(), yl->stride_sample))
  {
    const int nr = c->n_joints(), nf = full->n_joints();
    bool mono = true;
    for (int g = 1; g < nf; ++g) mono = mono && full->red_of[g] >= full->red_of[g - 1];
    if (mono)
    {
      for (int f = 0; f <= nr; ++f)
      {
        int g = 0;
        while (g < nf && full->red_of[g] < f) ++g;
        a.expand_first[f] = g;   // (f = nr: nf)
      }
      for (int i = 0; i < n; ++i) a.row_map[c->active[i]] = i;  // reduced joint -> the caller's input index
      expand_image = true;
    }
  }
  if (yl && (mode == RDYN_MODE_REGRESSOR || mode == RDYN_MODE_REGRESSOR_EXPAND || mode == RDYN_MODE_REGRESSOR_EXPAND_STAGED))
  {
    // the one-thread-per-sample kernel addresses a workgroup's 256 samples with 32-bit lane offsets: free strides must be
    // positive and keep 255 * stride_sample * 8 inside 32 bits (the presets of rdyn.h are far below that)
    if (yl->stride_sample < 1 || yl->stride_row < 1 || yl->stride_col < 1 || yl->stride_sample > (int64_t)0xFFFFFFFFll / (8 * 255))
    {
      rdyn_set_error("rdyn_regressor: strides must be positive and stride_sample below %lld doubles", (long long)((int64_t)0xFFFFFFFFll / (8 * 255)));
      return RDYN_ERR_INVALID_ARGUMENT;
    }
  }
  a.M = M;
  rec_strides(b, (int64_t)n * n, &a.m_ss, &a.m_se);
  // torque / inertia records in the drop-in layout: through the wave's LDS tile, whole lines (rdyn_record_stage.h)
  if ((mode == RDYN_MODE_TORQUE || mode == RDYN_MODE_INERTIA) && b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(tau, M))
    a.staged = mode == RDYN_MODE_INERTIA ? n * n : n;
  // Row-contiguous regressor layouts (stacked column-major, per-sample Eigen image) with sample-major inputs:
  // ceil(n/2) lanes per sample, 16-byte row-pair stores (k_rowpair_sweep) instead of 8-byte strided stores.
  const bool rowpair = mode == RDYN_MODE_REGRESSOR && yl && yl->stride_row == 1 && n >= 2 && n <= 10 &&
                       b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && b->n_samples * ((n + 1) / 2) < (int64_t)0xFFFFFF00ll;
  // the drop-in per-sample image (either input layout): one thread per sample, link blocks staged through LDS (rdyn_image.hip)
  // and the stacked column-major (N n) x P matrix (stride_sample == n): same kernel, column-major staging tile per link
  unsigned fix_mask = 0;
  bool mapped = false;
  const bool image = mode == RDYN_MODE_REGRESSOR && yl && image_route(c, yl, b->n_samples, Y, false, &fix_mask, &mapped) != 0;
  if (expand_image)
  {
    // (the chunk permutation of the per-sample images, see below)
    const unsigned grid = (unsigned)((b->n_samples + 63) / 64);
    auto gcd = [](unsigned x, unsigned y) { while (y) { const unsigned t = x % y; x = y; y = t; } return x; };
    unsigned m = 257;
    while (gcd(m, grid) != 1) ++m;
    a.blk_mul = (grid > 4 * m) ? m : 0;
    RDYN_HIP_TRY(rdyn_launch_image_sweep(c->n_joints(), 0u, a, (hipStream_t)b->stream, 2));
  }
  else if (image)
  {
    if (mapped)
    {
      // the swept chain: the sorted view when the input joints were listed out of chain order (same joints, rows in chain order)
      const rdyn_chain* const so = c->sorted ? c->sorted.get() : c;
      st = device_const(so, &a.chain);
      if (st != RDYN_OK) return st;
      for (int f = 0; f < RDYN_MAX_SWEPT_JOINTS; ++f) a.row_map[f] = -1;
      for (int r = 0; r < n; ++r) a.row_map[so->active[r]] = r < (int)so->row_input.size() ? so->row_input[r] : r;
    }
    // per-sample images: the workgroups visit the 64-sample chunks of the batch in a PERMUTED order (chunk = b * 257 mod grid), so that
    // the ~2 000 waves resident at a time write all over the output instead of one contiguous ~370 MB window of it.  Measured (round 6,
    // tools/probe_scatter.py, profiles/r6/probe_scatter.txt: ten 2.88 GB output allocations per process): 516-523 -> 450-455 us per 1e6
    // evaluations in half of the allocations, 537-547 -> 508-520 in most others, never slower; multipliers 17 .. 4097 alike.  The stacked
    // matrix (60 column fronts already) loses 2-5 % with it and keeps the workgroups in order.
    if (image_route(c, yl, b->n_samples, Y, false, &fix_mask, &mapped) == 1)
    {
      const unsigned grid = (unsigned)((b->n_samples + 63) / 64);
      auto gcd = [](unsigned x, unsigned y) { while (y) { const unsigned t = x % y; x = y; y = t; } return x; };
      unsigned m = 257;
      while (gcd(m, grid) != 1) ++m;
      a.blk_mul = grid > 4 * m ? m : 0;
    }
    RDYN_HIP_TRY(rdyn_launch_image_sweep(c->n_joints(), fix_mask, a, (hipStream_t)b->stream, mapped));
  }
  else if (rowpair)
  {
    // the kernel addresses Y with a 32-bit per-lane byte offset: split so that every launch spans < 4 GB of Y
    const int64_t span = (a.y_ss > 0 ? a.y_ss : 1) * 8;
    int64_t chunk = ((int64_t)0xF0000000ll / span) & ~(int64_t)255;
    if (chunk < 256) chunk = 256;
    for (int64_t s0 = 0; s0 < b->n_samples; s0 += chunk)
    {
      RdynSweepArgs p = a;
      p.n_samples = (b->n_samples - s0 < chunk) ? b->n_samples - s0 : chunk;
      p.q = a.q + s0 * a.in_ss;
      p.dq = a.dq + s0 * a.in_ss;
      p.ddq = a.ddq + s0 * a.in_ss;
      p.Y = a.Y + s0 * a.y_ss;
      if (a.tau) p.tau = a.tau + s0 * a.tau_ss;
      RDYN_HIP_TRY(rdyn_launch_rowpair_sweep(c->n_joints(), n, p, (hipStream_t)b->stream));
    }
  }
  else
    RDYN_HIP_TRY(rdyn_launch_local_sweep(c->n_joints(), mode, a, (hipStream_t)b->stream));
  return RDYN_OK;
}

// regressor / inertia of a chain with more input joints than the unrolled kernels sweep (no reduced companion): the run-time-length
// kernels of rdyn_long_local.hip -- rolled link and row loops, per-joint state in wave-private LDS
int run_long_local(const rdyn_chain* c, const rdyn_batch* b, int mode, double* tau, double* Y, const rdyn_regressor_layout* yl, double* M)
{
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  int st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  RdynLongLocalArgs a;
  memset(&a, 0, sizeof a);
  st = device_const_long(c, &a.chain_long);
  if (st != RDYN_OK) return st;
  const int n = c->n_active();
  a.q = b->q;
  a.dq = b->dq;
  a.ddq = b->ddq;
  a.n_samples = b->n_samples;
  rec_strides(b, n, &a.in_ss, &a.in_sj);
  a.tau = tau;
  a.tau_ss = a.in_ss;
  a.tau_sj = a.in_sj;
  a.Y = Y;
  if (yl)
  {
    if (yl->stride_sample < 1 || yl->stride_row < 1 || yl->stride_col < 1)
    {
      rdyn_set_error("rdyn_regressor: strides must be positive");
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    a.y_ss = yl->stride_sample;
    a.y_sr = yl->stride_row;
    a.y_sc = yl->stride_col;
    // row-contiguous layouts: every link's block through the wave's LDS tile, copied out 16 bytes per lane
    if (yl->stride_row == 1 && ((uintptr_t)Y & 15) == 0)
    {
      if (yl->stride_col == n && yl->stride_sample % 2 == 0 && yl->stride_sample >= (int64_t)n * 10 * c->n_joints()) a.stage = 1;
      else if (yl->stride_sample == n && yl->stride_col % 2 == 0 && yl->stride_col >= b->n_samples * n) a.stage = 2;
    }
  }
  a.n_active = n;
  a.M = M;
  rec_strides(b, (int64_t)n * n, &a.m_ss, &a.m_se);
  RDYN_HIP_TRY(rdyn_launch_long_local(mode, c->n_joints(), a, (hipStream_t)b->stream));
  return RDYN_OK;
}

}  // namespace

extern "C"
{

// a chain of more than RDYN_MAX_SWEPT_JOINTS joints whose input joints are too many for the companion: the joint torques read off the
// wrench recursion of the run-time-length kernels (primitives_impl.h:1264-1272; use_ddq = false: DDq = 0)
static int long_chain_torque(const rdyn_chain* c, const rdyn_batch* b, double* tau, bool use_ddq)
{
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  int st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  RdynKinExtArgs e;
  memset(&e, 0, sizeof e);
  st = device_const_long(c, &e.chain_long);
  if (st != RDYN_OK) return st;
  e.q = b->q;
  e.dq = b->dq;
  e.ddq = use_ddq ? b->ddq : nullptr;
  e.n_samples = b->n_samples;
  rec_strides(b, c->n_active(), &e.in_ss, &e.in_sj);
  e.tau = tau;
  e.tau_ss = e.in_ss;
  e.tau_sj = e.in_sj;
  e.staged = b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(tau);
  RDYN_HIP_TRY(rdyn_launch_long_ext(c->n_joints(), e, (hipStream_t)b->stream));
  return RDYN_OK;
}

int rdyn_joint_torque(const rdyn_chain* c, const rdyn_batch* b, double* tau)
{
  const bool by_wrench = c && c->long_chain() && !c->reduced;
  int st = check_batch(c, b, true, true, "rdyn_joint_torque", by_wrench ? LONG_KERNELS : LONG_COMPANION);
  if (st != RDYN_OK) return st;
  if (!tau && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_joint_torque: null output");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (by_wrench) return long_chain_torque(c, b, tau, true);
  return run_local(c, b, RDYN_MODE_TORQUE, tau, nullptr, nullptr, nullptr, true, true);
}

int rdyn_joint_torque_nonlinear(const rdyn_chain* c, const rdyn_batch* b, double* tau)
{
  const bool by_wrench = c && c->long_chain() && !c->reduced;
  int st = check_batch(c, b, true, false, "rdyn_joint_torque_nonlinear", by_wrench ? LONG_KERNELS : LONG_COMPANION);
  if (st != RDYN_OK) return st;
  if (!tau && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_joint_torque_nonlinear: null output");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (by_wrench) return long_chain_torque(c, b, tau, false);
  return run_local(c, b, RDYN_MODE_TORQUE, tau, nullptr, nullptr, nullptr, true, false);  // DDq = 0, primitives_impl.h:1287-1288
}

int rdyn_regressor(const rdyn_chain* c, const rdyn_batch* b, double* tau, double* Y, const rdyn_regressor_layout* yl)
{
  int st = check_batch(c, b, true, true, "rdyn_regressor", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (b->n_samples > 0 && (!Y || !yl))
  {
    rdyn_set_error("rdyn_regressor: null output or layout");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (c->long_chain() && !c->reduced) return run_long_local(c, b, RDYN_MODE_REGRESSOR, tau, Y, yl, nullptr);
  return run_local(c, b, RDYN_MODE_REGRESSOR, tau, Y, yl, nullptr, true, true);
}

int rdyn_joint_inertia(const rdyn_chain* c, const rdyn_batch* b, double* M)
{
  int st = check_batch(c, b, false, false, "rdyn_joint_inertia", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!M && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_joint_inertia: null output");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (c->long_chain() && !c->reduced) return run_long_local(c, b, RDYN_MODE_INERTIA, nullptr, nullptr, nullptr, M);
  return run_local(c, b, RDYN_MODE_INERTIA, nullptr, nullptr, nullptr, M, false, false);
}

// ---- derivatives of the joint torque: dtau/dq, dtau/dDq, M (rdyn_torque_deriv.hip) ------------------------------
// Chains the unrolled kernels sweep (long ones through their reduced companion: the same function of the inputs): one launch.  More than
// RDYN_MAX_SWEPT_JOINTS input joints: the rolled kernel for the two derivative matrices, k_long_inertia for M.
int rdyn_joint_torque_derivatives(const rdyn_chain* c, const rdyn_batch* b, double* dtau_dq, double* dtau_dv, double* M)
{
  int st = check_batch(c, b, true, true, "rdyn_joint_torque_derivatives", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (b->n_samples > 0 && !dtau_dq && !dtau_dv && !M)
  {
    rdyn_set_error("rdyn_joint_torque_derivatives: every output is null");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (b->n_samples == 0 || c->n_active() < 1) return RDYN_OK;
  const int n = c->n_active();
  const bool by_long = c->long_chain() && !c->reduced;
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  if (by_long && (dtau_dq || dtau_dv) && (st = long_deriv_lds_refusal(c, "rdyn_joint_torque_derivatives")) != RDYN_OK) return st;
  RdynTorqueDerivArgs a;
  memset(&a, 0, sizeof a);
  a.q = b->q;
  a.dq = b->dq;
  a.ddq = b->ddq;
  a.n_samples = b->n_samples;
  rec_strides(b, n, &a.in_ss, &a.in_sj);
  rec_strides(b, (int64_t)n * n, &a.m_ss, &a.m_se);
  a.dtau_dq = dtau_dq;
  a.dtau_dv = dtau_dv;
  a.M = M;
  if (!by_long)
  {
    const rdyn_chain* const sw = c->long_chain() ? c->reduced.get() : c;
    st = device_const(sw, &a.chain);
    if (st != RDYN_OK) return st;
    a.staged = (b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(dtau_dq, dtau_dv, M)) ? n * n : 0;
    RDYN_HIP_TRY(rdyn_launch_torque_derivatives(sw->n_joints(), a, (hipStream_t)b->stream));
    return RDYN_OK;
  }
  if (dtau_dq || dtau_dv)
  {
    st = device_const_long(c, &a.chain_long);
    if (st != RDYN_OK) return st;
    RDYN_HIP_TRY(rdyn_launch_long_torque_derivatives(c->n_joints(), a, (hipStream_t)b->stream));
  }
  if (M) return run_long_local(c, b, RDYN_MODE_INERTIA, nullptr, nullptr, nullptr, M);
  return RDYN_OK;
}

static int run_base(const rdyn_chain* c, const rdyn_batch* b, double* T_bt, double* T_links, double* J, double* tw, double* dtw,
                    int j_link = -1)
{
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  int st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  RdynKinArgs a;
  memset(&a, 0, sizeof a);
  st = c->long_chain() ? device_const_long(c, &a.chain_long) : device_const(c, &a.chain);
  if (st != RDYN_OK) return st;
  const int n = c->n_active(), L = c->n_joints() + 1;
  a.q = b->q;
  a.dq = (tw || dtw) ? b->dq : nullptr;
  a.ddq = dtw ? b->ddq : nullptr;
  a.n_samples = b->n_samples;
  rec_strides(b, n, &a.in_ss, &a.in_sj);
  int64_t se;
  a.T_bt = T_bt;
  rec_strides(b, 12, &a.tb_ss, &se);
  a.T_links = T_links;
  rec_strides(b, 12 * (int64_t)L, &a.tl_ss, &se);
  a.J = J;
  a.j_link = j_link < 0 ? c->n_joints() : j_link;
  rec_strides(b, 6 * (int64_t)n, &a.j_ss, &se);
  a.twists = tw;
  a.dtwists = dtw;
  rec_strides(b, 6 * (int64_t)L, &a.tw_ss, &se);
  a.out_se = se;
  a.n_active = n;
  // the drop-in layout: records leave through wave-private LDS in whole lines (rdyn_record_stage.h) when every output starts on a line
  a.staged = b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(T_bt, T_links, J, tw, dtw);
  if (c->long_chain())
  {
    for (int l = 0; l < a.j_link; ++l) a.j_up += c->host_joints[l].in_idx >= 0 ? 1 : 0;
    RDYN_HIP_TRY(rdyn_launch_long_base(a, (hipStream_t)b->stream));
  }
  else
    RDYN_HIP_TRY(rdyn_launch_base_sweep(c->n_joints(), a, (hipStream_t)b->stream));
  return RDYN_OK;
}

// ---- batched local inverse kinematics -------------------------------------------------------------------------
int rdyn_local_ik(const rdyn_chain* c, const rdyn_batch* b, const double* T_target, const double* weight, double toll,
                  int max_iterations, double* sol, int32_t* status, int32_t* iterations)
{
  return rdyn_local_ik_damped(c, b, T_target, weight, toll, 0.0, max_iterations, sol, status, iterations);
}

int rdyn_local_ik_damped(const rdyn_chain* c, const rdyn_batch* b, const double* T_target, const double* weight, double toll,
                         double damping, int max_iterations, double* sol, int32_t* status, int32_t* iterations)
{
  // a long chain with more input joints than its reduced companion holds (no companion) runs on the rolled kernel, rdyn_long_ik.hip
  const bool long_route = c && c->long_chain() && !c->reduced;
  int st = check_batch(c, b, false, false, "rdyn_local_ik", long_route ? LONG_KERNELS : LONG_COMPANION);  // batch->q = the seeds
  if (st != RDYN_OK) return st;
  if (b->n_samples > 0 && (!T_target || !sol))
  {
    rdyn_set_error("rdyn_local_ik: null target or solution pointer");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (max_iterations < 0 || !(toll >= 0.0) || !(damping >= 0.0))
  {
    rdyn_set_error("rdyn_local_ik: negative iteration cap, tolerance or damping");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  if (long_route)
  {
    RdynLongIkArgs a;
    memset(&a, 0, sizeof a);
    st = device_const_long(c, &a.chain_long);
    if (st != RDYN_OK) return st;
    a.T_target = T_target;
    rec_strides(b, 12, &a.tt_ss, &a.tt_se);
    a.seed = b->q;
    a.sol = sol;
    a.n_samples = b->n_samples;
    rec_strides(b, c->n_active(), &a.in_ss, &a.in_sj);
    for (int i = 0; i < 6; ++i) a.weight[i] = weight ? weight[i] : 1.0;
    // the QP variables: the moving input joints in chain order
    for (int j = 0; j < c->n_joints(); ++j)
    {
      const RdynJointConst& J = c->host_long.j[j];
      if (J.in_idx < 0 || J.type == RDYN_FIXED) continue;
      a.var_in[a.n_var] = J.in_idx;
      a.q_min[a.n_var] = c->q_min[j];
      a.q_max[a.n_var] = c->q_max[j];
      ++a.n_var;
    }
    a.toll = toll;
    a.damping = damping;
    a.max_iter = max_iterations;
    a.status = status;
    a.iterations = iterations;
    RDYN_HIP_TRY(rdyn_launch_long_ik(a, (hipStream_t)b->stream));
    return RDYN_OK;
  }
  RdynIkArgs a;
  memset(&a, 0, sizeof a);
  if (c->long_chain())
  {
    // the pose and the Jacobian of the tool need only the input joints: the reduced companion (the fixed frames folded into the
    // joint origins) is iterated, its tool frame followed by the constant frames behind the last input joint
    a.has_tail = 1;
    memcpy(a.tail_R, c->tail_R, sizeof a.tail_R);
    memcpy(a.tail_t, c->tail_t, sizeof a.tail_t);
    c = c->reduced.get();
  }
  st = device_const(c, &a.chain);
  if (st != RDYN_OK) return st;
  a.T_target = T_target;
  rec_strides(b, 12, &a.tt_ss, &a.tt_se);
  a.seed = b->q;
  a.sol = sol;
  a.n_samples = b->n_samples;
  rec_strides(b, c->n_active(), &a.in_ss, &a.in_sj);
  for (int i = 0; i < 6; ++i) a.weight[i] = weight ? weight[i] : 1.0;
  for (int j = 0; j < c->n_joints(); ++j)
  {
    a.q_min[j] = c->q_min[j];
    a.q_max[j] = c->q_max[j];
  }
  a.toll = toll;
  a.damping = damping;
  a.max_iter = max_iterations;
  a.status = status;
  a.iterations = iterations;
  // Staged launches when the per-pose results are available to carry the state: most poses settle within a few updates,
  // the rest would keep every wave alive for the whole cap.  The first launch runs everyone for 8 updates; every further
  // launch gathers the poses still running into dense waves and continues only those up to the next boundary (same
  // arithmetic per pose, rdyn_ik.hip: k_local_ik_resume).
  // (boundaries at 4 and 16 as well were measured slower: re-packing 42 % of the poses after 4 updates costs more than the
  // idle lanes it saves -- cap 8: 1.64 ms vs 1.11 ms)
  static const int kIkStages[] = {8};  // update counts after which the survivors are re-packed
  const int n_stages = (int)(sizeof kIkStages / sizeof kIkStages[0]);
  if (status && iterations)
  {
    int done = 0;  // updates every still-running pose has performed so far
    for (int k = 0; k <= n_stages; ++k)
    {
      const int upto = (k < n_stages && kIkStages[k] < max_iterations) ? kIkStages[k] : max_iterations;
      a.it_stage = done;  // 0: first launch (all poses, from the seeds); > 0: resume the poses stopped at `done` updates
      a.max_iter = upto;
      RDYN_HIP_TRY(rdyn_launch_local_ik(c->n_joints(), a, (hipStream_t)b->stream));
      done = upto;
      if (upto == max_iterations) break;
    }
    return RDYN_OK;
  }
  RDYN_HIP_TRY(rdyn_launch_local_ik(c->n_joints(), a, (hipStream_t)b->stream));
  return RDYN_OK;
}

int rdyn_frame_distance(int64_t n_pairs, const double* T_wa, const double* T_wb, int layout, int kind, double* distance, double* jacobian,
                        int device, void* stream)
{
  if (n_pairs < 0 || (layout != RDYN_LAYOUT_SAMPLE_MAJOR && layout != RDYN_LAYOUT_ELEMENT_MAJOR) || kind < 0 || kind > 2 ||
      (n_pairs > 0 && (!T_wa || !T_wb || !distance)) || (jacobian && kind != RDYN_FRAME_DISTANCE_QUAT_JAC))
  {
    rdyn_set_error("rdyn_frame_distance: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (n_pairs == 0) return RDYN_OK;
  DeviceGuard g;
  int st = g.enter(device);
  if (st != RDYN_OK) return st;
  RdynFrameDistanceArgs a;
  memset(&a, 0, sizeof a);
  rdyn_batch b;
  memset(&b, 0, sizeof b);
  b.n_samples = n_pairs;
  b.layout = layout;
  a.T_wa = T_wa;
  a.T_wb = T_wb;
  a.n = n_pairs;
  a.kind = kind;
  a.distance = distance;
  a.jacobian = jacobian;
  rec_strides(&b, 12, &a.t_ss, &a.t_se);
  rec_strides(&b, 6, &a.d_ss, &a.d_se);
  rec_strides(&b, 36, &a.j_ss, &a.j_se);
  RDYN_HIP_TRY(rdyn_launch_frame_distance(a, (hipStream_t)stream));
  return RDYN_OK;
}

// ---- split / jerk sweeps, external wrenches ---------------------------------------------------------------
int rdyn_twist_parts(const rdyn_chain* c, const rdyn_batch* b, const double* dddq, double* dtw_lin, double* dtw_nonlin, double* ddtw)
{
  int st = check_batch(c, b, dtw_nonlin || ddtw, dtw_lin || ddtw, "rdyn_twist_parts", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if ((!dtw_lin && !dtw_nonlin && !ddtw) || (ddtw && !dddq && b->n_samples > 0))
  {
    rdyn_set_error("rdyn_twist_parts: no output, or ddtwists without dddq");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  RdynKinExtArgs a;
  memset(&a, 0, sizeof a);
  st = c->long_chain() ? device_const_long(c, &a.chain_long) : device_const(c, &a.chain);
  if (st != RDYN_OK) return st;
  a.q = b->q;
  a.dq = b->dq;
  a.ddq = b->ddq;
  a.dddq = dddq;
  a.n_samples = b->n_samples;
  rec_strides(b, c->n_active(), &a.in_ss, &a.in_sj);
  rec_strides(b, 6 * (int64_t)(c->n_joints() + 1), &a.out_ss, &a.out_se);
  a.dtw_lin = dtw_lin;
  a.dtw_nonlin = dtw_nonlin;
  a.ddtw = ddtw;
  a.staged = b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(dtw_lin, dtw_nonlin, ddtw);
  if (c->long_chain())
    RDYN_HIP_TRY(rdyn_launch_long_ext(c->n_joints(), a, (hipStream_t)b->stream));
  else
    RDYN_HIP_TRY(rdyn_launch_base_ext(c->n_joints(), a, (hipStream_t)b->stream));
  return RDYN_OK;
}

int rdyn_jerk_parts(const rdyn_chain* c, const rdyn_batch* b, const double* dddq, double* ddtw_lin, double* ddtw_nonlin)
{
  int st = check_batch(c, b, ddtw_nonlin != nullptr, ddtw_nonlin != nullptr, "rdyn_jerk_parts", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if ((!ddtw_lin && !ddtw_nonlin) || (ddtw_lin && !dddq && b->n_samples > 0))
  {
    rdyn_set_error("rdyn_jerk_parts: no output, or the linear part without dddq");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  RdynKinExtArgs a;
  memset(&a, 0, sizeof a);
  st = c->long_chain() ? device_const_long(c, &a.chain_long) : device_const(c, &a.chain);
  if (st != RDYN_OK) return st;
  a.q = b->q;
  a.dq = ddtw_nonlin ? b->dq : nullptr;
  a.ddq = ddtw_nonlin ? b->ddq : nullptr;
  a.dddq = ddtw_lin ? dddq : nullptr;
  a.n_samples = b->n_samples;
  rec_strides(b, c->n_active(), &a.in_ss, &a.in_sj);
  rec_strides(b, 6 * (int64_t)(c->n_joints() + 1), &a.out_ss, &a.out_se);
  a.ddtw_lin = ddtw_lin;
  a.ddtw_nonlin = ddtw_nonlin;
  a.staged = b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(ddtw_lin, ddtw_nonlin);
  if (c->long_chain())
    RDYN_HIP_TRY(rdyn_launch_long_ext(c->n_joints(), a, (hipStream_t)b->stream));
  else
    RDYN_HIP_TRY(rdyn_launch_base_ext(c->n_joints(), a, (hipStream_t)b->stream));
  return RDYN_OK;
}

int rdyn_wrench(const rdyn_chain* c, const rdyn_batch* b, const double* ext, double* wrenches)
{
  int st = check_batch(c, b, true, true, "rdyn_wrench", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!wrenches && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_wrench: null output");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  RdynKinExtArgs a;
  memset(&a, 0, sizeof a);
  st = c->long_chain() ? device_const_long(c, &a.chain_long) : device_const(c, &a.chain);
  if (st != RDYN_OK) return st;
  a.q = b->q;
  a.dq = b->dq;
  a.ddq = b->ddq;
  a.n_samples = b->n_samples;
  rec_strides(b, c->n_active(), &a.in_ss, &a.in_sj);
  rec_strides(b, 6 * (int64_t)(c->n_joints() + 1), &a.out_ss, &a.out_se);
  a.wrench = wrenches;
  a.ext = ext;
  a.ext_ss = a.out_ss;
  a.ext_se = a.out_se;
  a.staged = b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(wrenches);
  a.ext_staged = a.staged && ext && ((uintptr_t)ext & 15u) == 0;
  if (c->long_chain())
    RDYN_HIP_TRY(rdyn_launch_long_ext(c->n_joints(), a, (hipStream_t)b->stream));
  else
    RDYN_HIP_TRY(rdyn_launch_base_ext(c->n_joints(), a, (hipStream_t)b->stream));
  return RDYN_OK;
}

int rdyn_joint_torque_ext(const rdyn_chain* c, const rdyn_batch* b, const double* ext, double* tau)
{
  int st = check_batch(c, b, true, true, "rdyn_joint_torque_ext", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if ((!tau || !ext) && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_joint_torque_ext: null argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  if (c->long_chain())
  {
    // the wrench recursion of the run-time-length kernels, the joint torques read off the link wrenches (primitives_impl.h:1264-1272)
    RdynKinExtArgs e;
    memset(&e, 0, sizeof e);
    st = device_const_long(c, &e.chain_long);
    if (st != RDYN_OK) return st;
    e.q = b->q;
    e.dq = b->dq;
    e.ddq = b->ddq;
    e.n_samples = b->n_samples;
    rec_strides(b, c->n_active(), &e.in_ss, &e.in_sj);
    e.tau = tau;
    e.tau_ss = e.in_ss;
    e.tau_sj = e.in_sj;
    e.ext = ext;
    rec_strides(b, 6 * (int64_t)(c->n_joints() + 1), &e.ext_ss, &e.ext_se);
    e.staged = b->layout == RDYN_LAYOUT_SAMPLE_MAJOR && lines_aligned(tau);
    RDYN_HIP_TRY(rdyn_launch_long_ext(c->n_joints(), e, (hipStream_t)b->stream));
    return RDYN_OK;
  }
  RdynSweepArgs a;
  memset(&a, 0, sizeof a);
  st = device_const(c, &a.chain);
  if (st != RDYN_OK) return st;
  a.q = b->q;
  a.dq = b->dq;
  a.ddq = b->ddq;
  a.n_samples = b->n_samples;
  rec_strides(b, c->n_active(), &a.in_ss, &a.in_sj);
  a.tau = tau;
  a.tau_ss = a.in_ss;
  a.tau_sj = a.in_sj;
  a.ext = ext;
  rec_strides(b, 6 * (int64_t)(c->n_joints() + 1), &a.ext_ss, &a.ext_se);
  RDYN_HIP_TRY(rdyn_launch_local_sweep(c->n_joints(), RDYN_MODE_TORQUE, a, (hipStream_t)b->stream));
  return RDYN_OK;
}

// ---- additive components ---------------------------------------------------------------------------------
int rdyn_components_columns(const rdyn_component* comps, int n_comps)
{
  if (!comps || n_comps < 0) return -1;
  int k = 0;
  for (int i = 0; i < n_comps; ++i) k += (comps[i].type == RDYN_COMP_FRICTION2) ? 3 : 2;
  return k;
}

int rdyn_components_regressor(const rdyn_component* comps, int n_comps, int n_active, const rdyn_batch* b, double* C,
                              const rdyn_regressor_layout* cl, double* tau_add)
{
  if (!comps || n_comps < 1 || n_comps > RDYN_MAX_COMPONENTS || n_active < 1 || !b || (!C && !tau_add) || (C && !cl))
  {
    rdyn_set_error("rdyn_components_regressor: invalid argument (1..%d components, an output, a layout)", RDYN_MAX_COMPONENTS);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (b->n_samples < 0 || (b->layout != RDYN_LAYOUT_SAMPLE_MAJOR && b->layout != RDYN_LAYOUT_ELEMENT_MAJOR) ||
      (b->n_samples > 0 && (!b->q || !b->dq)))
  {
    rdyn_set_error("Input data dimensions mismatch");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  RdynComponentArgs a;
  memset(&a, 0, sizeof a);
  int cst = fill_components(comps, n_comps, n_active, &a);
  if (cst != RDYN_OK) return cst;
  if (b->n_samples == 0) return RDYN_OK;
  DeviceGuard g;
  int st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  a.q = b->q;
  a.dq = b->dq;
  a.n_samples = b->n_samples;
  rec_strides(b, n_active, &a.in_ss, &a.in_sj);
  a.n_active = n_active;
  a.n_comps = n_comps;
  a.C = C;
  if (cl)
  {
    a.c_ss = cl->stride_sample;
    a.c_sr = cl->stride_row;
    a.c_sc = cl->stride_col;
  }
  a.tau = tau_add;
  RDYN_HIP_TRY(rdyn_launch_components(a, (hipStream_t)b->stream));
  return RDYN_OK;
}

// ---- mixed-chain batch ----------------------------------------------------------------------------------
struct rdyn_multi_plan
{
  int device = 0;
  struct Group
  {
    int n_joints = 0;
    unsigned fix_mask = 0;  // image / stacked groups only: chain joints that are not input joints
    int kind = 0;      // 0: one thread per sample, strided stores (any layout); 1: per-sample images, 2: stacked matrices (rdyn_image.hip)
    int n_items = 0;
    int64_t max_samples = 0;
    RdynSweepArgs* table = nullptr;  // device
  };
  std::vector<Group> groups;
  ~rdyn_multi_plan()  // also runs when creation fails half-way
  {
    DeviceGuard g;
    if (g.enter(device) == RDYN_OK)
      for (auto& grp : groups) (void)hipFree(grp.table);
  }
};

int rdyn_multi_plan_create(const rdyn_multi_item* items, int n_items, rdyn_multi_plan** out)
{
  if (!items || n_items < 1 || !out)
  {
    rdyn_set_error("rdyn_multi_plan_create: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  *out = nullptr;
  DeviceGuard g;
  int st = g.enter(items[0].batch.device);
  if (st != RDYN_OK) return st;
  std::unique_ptr<rdyn_multi_plan> plan(new rdyn_multi_plan());
  RDYN_HIP_TRY(hipGetDevice(&plan->device));
  std::map<int, std::vector<RdynSweepArgs>> by_nj;
  std::map<int, int64_t> max_n;
  for (int i = 0; i < n_items; ++i)
  {
    const rdyn_multi_item& it = items[i];
    st = check_batch(it.chain, &it.batch, true, true, "rdyn_multi_plan_create", LONG_NONE);
    if (st != RDYN_OK) return st;
    if (it.batch.n_samples > 0 && !it.Y)
    {
      rdyn_set_error("rdyn_multi_plan_create: item %d has a null regressor output", i);
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    if (it.batch.n_samples > 0 &&  // an empty item's strides are never used (its row stride is its sample count: 0)
        (it.y_layout.stride_sample < 1 || it.y_layout.stride_row < 1 || it.y_layout.stride_col < 1 ||
         it.y_layout.stride_sample > (int64_t)0xFFFFFFFFll / (8 * 255)))
    {
      rdyn_set_error("rdyn_multi_plan_create: item %d: strides must be positive and stride_sample below %lld doubles", i,
                     (long long)((int64_t)0xFFFFFFFFll / (8 * 255)));
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    RdynSweepArgs a;
    memset(&a, 0, sizeof a);
    st = device_const(it.chain, &a.chain);
    if (st != RDYN_OK) return st;
    a.q = it.batch.q;
    a.dq = it.batch.dq;
    a.ddq = it.batch.ddq;
    a.n_samples = it.batch.n_samples;
    rec_strides(&it.batch, it.chain->n_active(), &a.in_ss, &a.in_sj);
    a.tau = it.tau;
    a.tau_ss = a.in_ss;
    a.tau_sj = a.in_sj;
    a.Y = it.Y;
    a.y_ss = it.y_layout.stride_sample;
    a.y_sr = it.y_layout.stride_row;
    a.y_sc = it.y_layout.stride_col;
    const int nj = it.chain->n_joints();
    // one launch per (chain joints, fixed-joint pattern, kernel kind): row-contiguous layouts of chains of up to 8 input joints go
    // through the LDS-staged kernels (whole-line stores), the rest keeps the strided kernel.  Key = nj | mask << 8 | kind << 24.
    unsigned fix_mask = 0;
    const int kind = it.batch.n_samples > 0 ? image_route(it.chain, &it.y_layout, it.batch.n_samples, it.Y, true, &fix_mask) : 0;
    const int key = nj | ((kind ? (int)fix_mask : 0) << 8) | (kind << 24);
    by_nj[key].push_back(a);
    if (a.n_samples > max_n[key]) max_n[key] = a.n_samples;
  }
  for (auto& kv : by_nj)
  {
    rdyn_multi_plan::Group grp;
    grp.n_joints = kv.first & 0xFF;
    grp.fix_mask = (unsigned)(kv.first >> 8) & 0xFFFFu;
    grp.kind = kv.first >> 24;
    grp.n_items = (int)kv.second.size();
    grp.max_samples = max_n[kv.first];
    RDYN_HIP_TRY(hipMalloc((void**)&grp.table, sizeof(RdynSweepArgs) * kv.second.size()));
    plan->groups.push_back(grp);
    RDYN_HIP_TRY(hipMemcpy(grp.table, kv.second.data(), sizeof(RdynSweepArgs) * kv.second.size(), hipMemcpyHostToDevice));
  }
  *out = plan.release();
  return RDYN_OK;
}

int rdyn_multi_plan_regressor(const rdyn_multi_plan* plan, void* stream)
{
  if (!plan)
  {
    rdyn_set_error("rdyn_multi_plan_regressor: null plan");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g;
  int st = g.enter(plan->device);
  if (st != RDYN_OK) return st;
  for (const auto& grp : plan->groups)
  {
    if (grp.kind)
      RDYN_HIP_TRY(rdyn_launch_image_sweep_multi(grp.n_joints, grp.fix_mask, grp.kind == 2, grp.table, grp.n_items, grp.max_samples, (hipStream_t)stream));
    else
      RDYN_HIP_TRY(rdyn_launch_local_sweep_multi(grp.n_joints, RDYN_MODE_REGRESSOR, grp.table, grp.n_items, grp.max_samples, (hipStream_t)stream));
  }
  return RDYN_OK;
}

void rdyn_multi_plan_destroy(rdyn_multi_plan* plan)
{
  delete plan;  // the destructor releases the device tables
}

int rdyn_evaluate_all(const rdyn_chain* c, const rdyn_batch* b, const rdyn_all_outputs* o)
{
  // (a long chain goes through the single-purpose calls below: each one decides for itself what it serves, so that a request for
  // frames / Jacobian / twists / torques of a chain whose inertia and regressor are not served is answered, not refused as a whole)
  int st = check_batch(c, b, true, true, "rdyn_evaluate_all", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!o)
  {
    rdyn_set_error("rdyn_evaluate_all: null outputs");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (b->n_samples == 0) return RDYN_OK;
  const int n = c->n_active(), nJ = c->n_joints(), L = nJ + 1;
  const rdyn_regressor_layout image = {(int64_t)n * 10 * nJ, 1, n};
  const rdyn_regressor_layout* const yl = o->y_layout ? o->y_layout : &image;
  if (c->long_chain())
  {
    // a chain longer than the unrolled kernels sweep: the single-purpose launches (companion + run-time-length kernels), same stream
    if (o->T_links && (st = rdyn_transformation(c, b, nullptr, o->T_links)) != RDYN_OK) return st;
    if (o->J && (st = rdyn_jacobian(c, b, o->J)) != RDYN_OK) return st;
    if ((o->twists || o->dtwists) && (st = rdyn_twist(c, b, o->twists, o->dtwists)) != RDYN_OK) return st;
    if (o->tau && (st = rdyn_joint_torque(c, b, o->tau)) != RDYN_OK) return st;
    if (o->tau_nonlinear && (st = rdyn_joint_torque_nonlinear(c, b, o->tau_nonlinear)) != RDYN_OK) return st;
    if (o->M && (st = rdyn_joint_inertia(c, b, o->M)) != RDYN_OK) return st;
    if (o->Y && (st = rdyn_regressor(c, b, nullptr, o->Y, yl)) != RDYN_OK) return st;
    return RDYN_OK;
  }
  if (o->Y && (yl->stride_sample < 1 || yl->stride_row < 1 || yl->stride_col < 1 || yl->stride_sample > (int64_t)0xFFFFFFFFll / (8 * 255)))
  {
    rdyn_set_error("rdyn_evaluate_all: regressor strides must be positive and stride_sample below %lld doubles", (long long)((int64_t)0xFFFFFFFFll / (8 * 255)));
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  const RdynChainConst* dc = nullptr;
  st = device_const(c, &dc);
  if (st != RDYN_OK) return st;
  RdynAllArgs a;
  memset(&a, 0, sizeof a);
  a.n_samples = b->n_samples;
  int64_t se;
  auto kin = [&](RdynKinArgs& k) {
    k.chain = dc;
    k.q = b->q;
    k.dq = b->dq;
    k.ddq = b->ddq;
    k.n_samples = b->n_samples;
    rec_strides(b, n, &k.in_ss, &k.in_sj);
    rec_strides(b, 12 * (int64_t)L, &k.tl_ss, &se);
    rec_strides(b, 6 * (int64_t)n, &k.j_ss, &se);
    rec_strides(b, 6 * (int64_t)L, &k.tw_ss, &se);
    k.out_se = se;
    k.j_link = nJ;
  };
  kin(a.frames);
  a.frames.T_links = o->T_links;
  kin(a.jacobian);
  a.jacobian.J = o->J;
  kin(a.twists);
  a.twists.twists = o->twists;
  a.twists.dtwists = o->dtwists;
  auto sweep = [&](RdynSweepArgs& w, bool use_ddq) {
    w.chain = dc;
    w.q = b->q;
    w.dq = b->dq;
    w.ddq = use_ddq ? b->ddq : nullptr;
    w.n_samples = b->n_samples;
    rec_strides(b, n, &w.in_ss, &w.in_sj);
    w.tau_ss = w.in_ss;
    w.tau_sj = w.in_sj;
    rec_strides(b, (int64_t)n * n, &w.m_ss, &w.m_se);
  };
  sweep(a.torque, true);
  a.torque.tau = o->tau;
  sweep(a.torque_nl, false);  // DDq = 0, primitives_impl.h:1287-1288
  a.torque_nl.tau = o->tau_nonlinear;
  sweep(a.inertia, false);
  a.inertia.dq = nullptr;
  a.inertia.M = o->M;
  sweep(a.regressor, true);
  a.regressor.Y = o->Y;
  a.regressor.y_ss = yl->stride_sample;
  a.regressor.y_sr = yl->stride_row;
  a.regressor.y_sc = yl->stride_col;
  RDYN_HIP_TRY(rdyn_launch_sample_all(nJ, a, (hipStream_t)b->stream));
  return RDYN_OK;
}

int rdyn_transformation(const rdyn_chain* c, const rdyn_batch* b, double* T_bt, double* T_links)
{
  int st = check_batch(c, b, false, false, "rdyn_transformation", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!T_bt && !T_links && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_transformation: null outputs");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  return run_base(c, b, T_bt, T_links, nullptr, nullptr, nullptr);
}

int rdyn_jacobian(const rdyn_chain* c, const rdyn_batch* b, double* J)
{
  int st = check_batch(c, b, false, false, "rdyn_jacobian", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!J && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_jacobian: null output");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  return run_base(c, b, nullptr, nullptr, J, nullptr, nullptr);
}

int rdyn_jacobian_link(const rdyn_chain* c, const rdyn_batch* b, int link_index, double* J)
{
  int st = check_batch(c, b, false, false, "rdyn_jacobian_link", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (link_index < 0 || link_index > c->n_joints())
  {
    rdyn_set_error("link index %d is not member of the chain", link_index);  // primitives_impl.h:960
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (!J && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_jacobian_link: null output");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  return run_base(c, b, nullptr, nullptr, J, nullptr, nullptr, link_index);
}

int rdyn_twist(const rdyn_chain* c, const rdyn_batch* b, double* twists, double* dtwists)
{
  int st = check_batch(c, b, true, dtwists != nullptr, "rdyn_twist", LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!twists && !dtwists && b->n_samples > 0)
  {
    rdyn_set_error("rdyn_twist: null outputs");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  return run_base(c, b, nullptr, nullptr, nullptr, twists, dtwists);
}

}  // extern "C"
