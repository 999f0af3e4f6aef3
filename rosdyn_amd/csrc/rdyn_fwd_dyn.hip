// rdyn_fwd_dyn.hip -- batched forward dynamics: ddq = M(q)^-1 (tau - h(q, dq)) (rdyn_forward_dynamics; no counterpart in the
// reference, defined by getJointInertia, primitives_impl.h:1357-1379, and getJointTorqueNonLinearPart, :1274-1293).
//
//   k_fwd_dyn<NJ>   chains the unrolled kernels sweep (1 .. RDYN_MAX_SWEPT_JOINTS joints): ONE launch, one lane per sample, nothing
//     but the inputs and the result touches memory.
//       forward   the local-frame sweep of rdyn_local_sweep_body.inc's torque mode with DDq = 0: w, vl, al, acc per link and the
//                 link's net wrench about its origin (getWrench, :1240-1250); sin q / 1 - cos q are kept per joint (2 NJ doubles),
//                 the wrenches wait for the backward pass (6 NJ doubles)
//       backward  composite rigid bodies: the spatial inertia of everything downstream of joint j is ten numbers in link j + 1's
//                 frame (m, h = m c, I about the link origin), carried to the parent by the rebuilt joint transform together with the
//                 bias wrench; h_j = S_j . (wrench), and column j of M is S_l . (Ic_j S_j) for the joints l <= j upstream: the six
//                 numbers Ic_j S_j of every column already started ride along into the parent frame (6 (NJ - j) doubles while the
//                 wrenches of the links passed are released).  The packed lower triangle of M is NJ (NJ + 1) / 2 <= 55 doubles.
//       solve     unrolled Cholesky M = L L' in place, two triangular solves.  A joint that is not an input joint is locked at 0: its
//                 row and column are replaced by the identity's and its right-hand side by 0, so the factorisation stays branch-free.
//     The O(n) articulated-body algorithm keeps a 6 x 6 articulated inertia (21 doubles) per link alive between its second and third
//     pass: 420 registers at 10 joints against 110 for the packed M, and at n <= 10 the factorisation is ~n^3 / 6 <= 170 fma.
//   k_fwd_solve     more than RDYN_MAX_SWEPT_JOINTS input joints: k_long_inertia (rdyn_long_local.hip) and the wrench recursion
//     (rdyn_long_kin.hip) write an element-major chunk image [M | h] (image[e][s]: every access of a wave is 512 contiguous bytes);
//     this kernel factorises it in place, one lane per sample, left-looking by columns: row j of L and the solution vector sit in
//     wave-private LDS ([k][lane]: a lane reads and writes its own column, no barrier), so the inner product of an entry costs one
//     global (L2 / Infinity Cache) and one LDS load per term.
// Status: 1 solved; -1 a Cholesky pivot (the squared diagonal entry of L, as in rdyn_ik.hip) at most 1e-10 trace(M) -- the sample's ddq
// is quiet NaN.
#include <hip/hip_runtime.h>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_fwd_dyn_body.h"
#include "rdyn_component_row.h"
#include "rdyn_launch_util.h"
#include <type_traits>

namespace
{
template <int NJ>
__global__ __launch_bounds__(64) void k_fwd_dyn(const RdynFwdDynArgs a)
{
#define RDYN_FWD_KERNEL_RHS(rhs)
#define RDYN_FWD_LINK_WRENCH(f, R, t, fo, no)
#include "rdyn_fwd_dyn_kernel.inc"
#undef RDYN_FWD_LINK_WRENCH
#undef RDYN_FWD_KERNEL_RHS
}

__device__ __forceinline__ const RdynFwdSolveArgs& solve_args(const RdynFwdSolveArgs& a) { return a; }
__device__ __forceinline__ const RdynFwdSolveArgs& solve_args(const RdynFwdSolveCompArgs& a) { return a.s; }

// element (i, j) of the lane's M at image[(i n + j) ld], h_i at image[(n n + i) ld]; both triangles of M are present, the lower one is used
// Args = RdynFwdSolveArgs: the torque is tau; RdynFwdSolveCompArgs: tau - tau_c at the sample's (q, dq), which the lane reads the way it
// reads tau (rdyn_forward_dynamics_components, the stages of rdyn_rollout_components)
template <class Args>
__global__ __launch_bounds__(64) void k_fwd_solve(const Args aa)
{
  constexpr bool COMPS = std::is_same<Args, RdynFwdSolveCompArgs>::value;
  const RdynFwdSolveArgs& a = solve_args(aa);
  extern __shared__ __attribute__((aligned(16))) double fwd_lds[];  // [2][n][64]: row j of L | the solution vector
  const int n = a.n;
  const int lane = threadIdx.x;
  const int64_t sl = (int64_t)blockIdx.x * 64 + lane;  // sample of the chunk
  if (sl >= a.n_samples) return;
  const int64_t ld = a.ld;
  double* const G = a.image + sl;
  double* const row = fwd_lds + lane;
  double* const y = fwd_lds + n * 64 + lane;
  const double* tp = a.tau + sl * a.in_ss;  // (may alias ddq: read whole before the first store)
  double* const op = a.ddq + sl * a.in_ss;

  double trace = 0.0;
#pragma unroll 4
  for (int i = 0; i < n; ++i)
  {
    trace += G[(int64_t)(i * n + i) * ld];
    double t = tp[i * a.in_sj];
    if constexpr (COMPS) t -= joint_component_torque(aa.t, i, aa.q[sl * a.in_ss + i * a.in_sj], aa.dq[sl * a.in_ss + i * a.in_sj]);
    y[i * 64] = t - G[(int64_t)(n * n + i) * ld];
  }
  const double floor = RDYN_FWD_PIVOT_FLOOR * trace;
  bool ok = true;
#pragma unroll 1
  for (int j = 0; j < n; ++j)
  {
    double d = G[(int64_t)(j * n + j) * ld];
#pragma unroll 4
    for (int k = 0; k < j; ++k)
    {
      const double l = G[(int64_t)(j * n + k) * ld];
      row[k * 64] = l;
      d = fma(-l, l, d);
    }
    ok = ok && d > floor;
    const double inv = 1.0 / sqrt(d);
    G[(int64_t)(j * n + j) * ld] = inv;
#pragma unroll 1
    for (int i = j + 1; i < n; ++i)
    {
      double* const gi = G + (int64_t)(i * n) * ld;
      double v = gi[(int64_t)j * ld];
#pragma unroll 4
      for (int k = 0; k < j; ++k) v = fma(-gi[(int64_t)k * ld], row[k * 64], v);
      gi[(int64_t)j * ld] = v * inv;
    }
  }
#pragma unroll 1
  for (int i = 0; i < n; ++i)
  {
    const double* const gi = G + (int64_t)(i * n) * ld;
    double v = y[i * 64];
#pragma unroll 4
    for (int k = 0; k < i; ++k) v = fma(-gi[(int64_t)k * ld], y[k * 64], v);
    y[i * 64] = v * gi[(int64_t)i * ld];
  }
#pragma unroll 1
  for (int i = n - 1; i >= 0; --i)
  {
    double v = y[i * 64];
#pragma unroll 4
    for (int k = i + 1; k < n; ++k) v = fma(-G[(int64_t)(k * n + i) * ld], y[k * 64], v);
    y[i * 64] = v * G[(int64_t)(i * n + i) * ld];
  }
  if (a.status) a.status[sl] = ok ? 1 : -1;
  const double qnan = __builtin_nan("");
#pragma unroll 4
  for (int i = 0; i < n; ++i) op[i * a.in_sj] = ok ? y[i * 64] : qnan;
}

template <int NJ>
hipError_t launch_fwd_nj(const RdynFwdDynArgs& a, hipStream_t st)
{
  const size_t lds = a.staged ? (size_t)64 * (size_t)(a.staged | 1) * 8 : 0;
  hipLaunchKernelGGL((k_fwd_dyn<NJ>), dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_forward_dynamics(int n_joints, const RdynFwdDynArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
#define CALL(N) launch_fwd_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

hipError_t rdyn_launch_forward_solve(const RdynFwdSolveArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
  if (a.n < 1 || a.n > RDYN_MAX_JOINTS || a.ld < a.n_samples) return hipErrorInvalidValue;
  const size_t lds = (size_t)2 * a.n * 64 * sizeof(double);  // <= 32 KB
  hipLaunchKernelGGL(k_fwd_solve<RdynFwdSolveArgs>, dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}

hipError_t rdyn_launch_forward_solve_components(const RdynFwdSolveCompArgs& a, hipStream_t st)
{
  if (a.s.n_samples <= 0) return hipSuccess;
  if (a.s.n < 1 || a.s.n > RDYN_MAX_JOINTS || a.s.ld < a.s.n_samples || a.t.n_comps < 0 || a.t.n_comps > RDYN_MAX_COMPONENTS) return hipErrorInvalidValue;
  const size_t lds = (size_t)2 * a.s.n * 64 * sizeof(double);  // <= 32 KB
  hipLaunchKernelGGL(k_fwd_solve<RdynFwdSolveCompArgs>, dim3((unsigned)((a.s.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
