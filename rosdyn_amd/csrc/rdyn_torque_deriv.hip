// rdyn_torque_deriv.hip -- batched derivatives of the inverse dynamics (rdyn_joint_torque_derivatives; no counterpart in the reference,
// defined by getJointTorque, primitives_impl.h:1264-1272, and getJointInertia, :1357-1379):
//     dtau_dq(i, k) = d tau_i / d q_k,   dtau_dv(i, k) = d tau_i / d Dq_k,   M(i, k) = d tau_i / d DDq_k
// of exactly the function the torque sweep of rdyn_local_sweep_body.inc evaluates (input joints in any order, joints that are not input
// joints locked at 0, fixed joints, gravity).
//
// Algorithm: a forward-mode tangent of the local-frame RNEA, one input joint (= one column of both matrices) at a time.
//   primal    the torque sweep with its backward pass: per link the velocity state w, vl, al, acc (12 doubles) and, after the backward
//             accumulation, the wrench Fc, Nc transmitted through the link's joint (6 doubles); sin q / 1 - cos q and Dq per joint.
//   seed      every quantity of link k is R_k' x plus terms along the joint axis u, and d R_k' / d q_k = -[u]x R_k', so
//               revolute   d(w, vl, al, acc) / d q_k = (w, vl, al, acc)_k x u          d / d Dq_k: dw = u, dal = w_k x u, dacc = vl_k x u
//               prismatic  dvl = w_k x u, dacc = al_k x u (the rest 0)                 d / d Dq_k: dvl = u, dacc = w_k x u
//             -- no transcendental and nothing of the parent link is needed.
//   forward   the tangent state rides down the chain through the rebuilt joint transforms (linear: the transforms of the joints
//             downstream do not depend on q_k), picks up (dvl x u) Dq_f / (dw x u) Dq_f at every joint, and leaves the tangent of every
//             link's net wrench (6 doubles per link downstream of k).
//   backward  the tangent wrenches are accumulated towards the base; row i of the column is S_i . (accumulated tangent wrench).
//             Passing joint k itself the transform's own derivative joins in: d(R F)/d q_k = R (u x F), the translation of a prismatic
//             joint gives u x Fc_k in the moment -- the cross product of the joint axis with the PRIMAL wrench through joint k.
//   Every entry is stored (or dropped into the wave's record tile) the moment it is known: nothing of the n x n outputs stays in
//   registers.  O(n^2) per sample like the inertia, no division, one sincos per revolute joint.
//   M         the composite-rigid-body pass of rdyn_fwd_dyn_body.inc (spatial inertia of everything downstream of joint j carried to the parent
//             with the columns already started), entries stored as they appear; skipped when M is null.
//
//   k_torque_deriv<NJ>    1 .. RDYN_MAX_SWEPT_JOINTS chain joints, everything unrolled, one lane per sample, ONE launch.  Chain constants
//     by scalar loads.  Sample-major records of a full wave go through the wave's LDS tile (64 (n n | 1) doubles, one output after the
//     other) in whole lines when the host found the outputs line-aligned (rdyn_record_stage.h); otherwise 8-byte stores.  Element-major
//     stores are 512 contiguous bytes per instruction.
//   k_long_torque_deriv   more input joints than that (chains without a reduced companion): the same recursion with rolled loops, the
//     27 per-joint values in wave-private LDS ([value][joint][lane]).  27 nj doubles per sample do not fit 64 lanes beside each other
//     beyond 11 joints: the workgroup is 64, 32 or 16 lanes, whichever keeps most samples resident in the LDS the device reports
//     (hipDeviceAttributeMaxSharedMemoryPerBlock: the 160 KB of a CU on gfx950, where 32 joints x 16 lanes ask for 108 KB).
#include <hip/hip_runtime.h>
#include <atomic>
#include <type_traits>
#include "rdyn_device.h"
#include "rdyn_devmath.h"
#include "rdyn_kernels.h"
#include "rdyn_record_stage.h"
#include "rdyn_launch_util.h"
#include "rdyn_long_common.h"
#include "rdyn_joint_step.h"
#include "rdyn_tangent_step.h"

namespace
{
template <int NJ>
__global__ __launch_bounds__(64) void k_torque_deriv(const RdynTorqueDerivArgs a)
{
  ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x;
  const int64_t s_wave = (int64_t)blockIdx.x * 64;
  const int64_t s = s_wave + lane;
  if (s >= a.n_samples) return;
  const bool stg = a.staged && a.n_samples - s_wave >= 64;  // wave-uniform: a full wave's records leave in whole lines
  const int n = c->n_active;
  const double* __restrict__ qp = a.q + s * a.in_ss;
  const double* __restrict__ dqp = a.dq + s * a.in_ss;
  const double* __restrict__ ddqp = a.ddq + s * a.in_ss;
  SmallRecords sm;
  if (stg)
  {
    extern __shared__ __attribute__((aligned(16))) char td_stage_lds[];
    sm.init(td_stage_lds, n * n, lane);
  }

  // ---- primal forward sweep: the state of every link, its net wrench
  double sv0[NJ], sv1[NJ], dqs[NJ];
  V3 W[NJ], VL[NJ], AL[NJ], AC[NJ], Fc[NJ], Nc[NJ];
  const bool want_d = a.dtau_dq || a.dtau_dv;  // wave-uniform
  if (want_d)
  {
    V3 w = mk(0, 0, 0), vl = mk(0, 0, 0), al = mk(0, 0, 0);
    V3 acc = mk(-c->g[0], -c->g[1], -c->g[2]);  // base "acceleration" -g
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      JointRef J = c->j[f];
      const int idx = J.in_idx;
      double qf = 0.0, dqf = 0.0, ddqf = 0.0;
      if (idx >= 0)
      {
        const int64_t o = idx * a.in_sj;
        qf = qp[o];
        dqf = dqp[o];
        ddqf = ddqp[o];
      }
      joint_sincos_state(J.type, qf, sv0[f], sv1[f]);
      dqs[f] = dqf;
      double R[9];
      V3 t;
      joint_transform(J, sv0[f], sv1[f], R, t);
      primal_step(J, R, t, dqf, ddqf, w, vl, al, acc);
      W[f] = w; VL[f] = vl; AL[f] = al; AC[f] = acc;
      link_wrench(J, w, vl, al, acc, Fc[f], Nc[f]);
    }
    // ---- primal backward pass: Fc, Nc[f] = the wrench through joint f (everything downstream), about link f + 1's origin, own frame
#pragma unroll
    for (int f = NJ - 1; f >= 1; --f)
    {
      double R[9];
      V3 t;
      joint_transform(c->j[f], sv0[f], sv1[f], R, t);
      const V3 Fp = rot(R, Fc[f]);
      Nc[f - 1] = Nc[f - 1] + rot(R, Nc[f]) + cross(t, Fp);
      Fc[f - 1] = Fc[f - 1] + Fp;
    }

    // ---- one column per input joint: KIND 0 d / d q_k, KIND 1 d / d Dq_k
    auto columns = [&](auto kind_tag, double* out) {
      constexpr int KIND = decltype(kind_tag)::value;
      double* const op = out + s * a.m_ss;
#pragma unroll
      for (int k = 0; k < NJ; ++k)
      {
        JointRef Jk = c->j[k];
        const int col = Jk.in_idx;
        if (col < 0) continue;
        V3 dFo[NJ], dNo[NJ];  // (entries k .. NJ - 1 are used)
        {
          Tangent d = tangent_seed(KIND, Jk.type, ld3(Jk.u), W[k], VL[k], AL[k], AC[k]);
          tangent_wrench(Jk, W[k], VL[k], d, dFo[k], dNo[k]);
#pragma unroll
          for (int f = k + 1; f < NJ; ++f)
          {
            JointRef J = c->j[f];
            double R[9];
            V3 t;
            joint_transform(J, sv0[f], sv1[f], R, t);
            tangent_step(J, R, t, dqs[f], d);
            tangent_wrench(J, W[f], VL[f], d, dFo[f], dNo[f]);
          }
        }
        V3 dF = mk(0, 0, 0), dN = mk(0, 0, 0);
#pragma unroll
        for (int f = NJ - 1; f >= 0; --f)
        {
          JointRef J = c->j[f];
          const int type = J.type;
          const V3 u = ld3(J.u);
          if (f >= k)
          {
            dF = dF + dFo[f];
            dN = dN + dNo[f];
          }
          const int row = J.in_idx;
          if (row >= 0)
          {
            double v = 0.0;
            if (type == RDYN_REVOLUTE) v = dot(u, dN);
            else if (type == RDYN_PRISMATIC) v = dot(u, dF);
            const int e = row + n * col;
            if (stg) sm.put(e, v);
            else op[e * a.m_se] = v;
          }
          if (f == 0) break;
          if (KIND == 0 && f == k)
          {
            // the derivative of joint k's own transform applied to the primal wrench it transmits
            if (type == RDYN_REVOLUTE)
            {
              dF = dF + cross(u, Fc[k]);
              dN = dN + cross(u, Nc[k]);
            }
            else if (type == RDYN_PRISMATIC)
              dN = dN + cross(u, Fc[k]);
          }
          double R[9];
          V3 t;
          joint_transform(J, sv0[f], sv1[f], R, t);
          const V3 Fp = rot(R, dF);
          dN = rot(R, dN) + cross(t, Fp);
          dF = Fp;
        }
      }
      if (stg) sm.copy_out(out + s_wave * a.m_ss, lane);
    };
    if (a.dtau_dq) columns(std::integral_constant<int, 0>(), a.dtau_dq);
    if (a.dtau_dv) columns(std::integral_constant<int, 1>(), a.dtau_dv);
  }

  if (!a.M) return;
  // ---- M by composite rigid bodies (rdyn_fwd_dyn_body.inc): needs sin q / 1 - cos q only
  if (!want_d)
  {
#pragma unroll
    for (int f = 0; f < NJ; ++f)
    {
      JointRef J = c->j[f];
      const int idx = J.in_idx;
      const double qf = idx >= 0 ? qp[idx * a.in_sj] : 0.0;
      joint_sincos_state(J.type, qf, sv0[f], sv1[f]);
    }
  }
  {
    double* const mp = a.M + s * a.m_ss;
    V3 cF[NJ], cN[NJ];  // column f: the momentum of composite body f under joint f's unit twist, in the current frame
    double cm = 0.0, cI[6] = {0, 0, 0, 0, 0, 0};
    V3 ch = mk(0, 0, 0);
#pragma unroll
    for (int j = NJ - 1; j >= 0; --j)
    {
      JointRef J = c->j[j];
      const int type = J.type;
      const int row = J.in_idx;
      const RDYN_CONST_AS double* pi = J.pi;
      cm += pi[0];
      ch = ch + ld3(pi + 1);
#pragma unroll
      for (int i = 0; i < 6; ++i) cI[i] += pi[4 + i];
      const V3 u = ld3(J.u);
      // momentum under the unit twist (lin, ang): F = m lin + ang x h, N = h x lin + I ang
      if (type == RDYN_REVOLUTE)
      {
        cF[j] = cross(u, ch);
        cN[j] = symv(cI, u);
      }
      else if (type == RDYN_PRISMATIC)
      {
        cF[j] = mk(cm * u.x, cm * u.y, cm * u.z);
        cN[j] = cross(ch, u);
      }
      else
      {
        cF[j] = mk(0, 0, 0);
        cN[j] = mk(0, 0, 0);
      }
#pragma unroll
      for (int f = j; f < NJ; ++f)
      {
        const int col = c->j[f].in_idx;
        if (row < 0 || col < 0) continue;
        double v = 0.0;
        if (type == RDYN_REVOLUTE) v = dot(u, cN[f]);
        else if (type == RDYN_PRISMATIC) v = dot(u, cF[f]);
        if (stg)
        {
          sm.put(row + n * col, v);
          sm.put(col + n * row, v);
        }
        else
        {
          mp[(row + n * col) * a.m_se] = v;
          mp[(col + n * row) * a.m_se] = v;
        }
      }
      if (j == 0) break;
      // into the parent's frame: x_parent = R x + t
      double R[9];
      V3 t;
      joint_transform(J, sv0[j], sv1[j], R, t);
#pragma unroll
      for (int f = j; f < NJ; ++f)
      {
        const V3 Fp = rot(R, cF[f]);
        cN[f] = rot(R, cN[f]) + cross(t, Fp);
        cF[f] = Fp;
      }
      ch = composite_to_parent(R, t, cm, ch, cI);
    }
    if (stg) sm.copy_out(a.M + s_wave * a.m_ss, lane);
  }
}

// ---- more input joints than the unrolled kernel sweeps ---------------------------------------------------------------------------------
enum { TD_W = 0, TD_VL = 3, TD_AL = 6, TD_AC = 9, TD_FC = 12, TD_NC = 15, TD_S0 = 18, TD_S1 = 19, TD_DQ = 20, TD_DF = 21, TD_DN = 24, TD_VALUES = 27 };

__global__ __launch_bounds__(64) void k_long_torque_deriv(const RdynTorqueDerivArgs a)
{
  extern __shared__ __attribute__((aligned(16))) double td_joint_lds[];  // [TD_VALUES][nj][lanes]
  LongChainPtr c = as_const_long(a.chain_long);
  const int nj = c->n_joints, n = c->n_active;
  const int lanes = blockDim.x, lane = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * lanes + lane;
  if (s >= a.n_samples) return;
  const JointState js = {td_joint_lds + lane, nj, lanes};
  const double* __restrict__ qp = a.q + s * a.in_ss;
  const double* __restrict__ dqp = a.dq + s * a.in_ss;
  const double* __restrict__ ddqp = a.ddq + s * a.in_ss;

  {
    V3 w = mk(0, 0, 0), vl = mk(0, 0, 0), al = mk(0, 0, 0);
    V3 acc = mk(-c->g[0], -c->g[1], -c->g[2]);
#pragma unroll 1
    for (int f = 0; f < nj; ++f)
    {
      JointRef J = c->j[f];
      const int idx = J.in_idx;
      double qf = 0.0, dqf = 0.0, ddqf = 0.0;
      if (idx >= 0)
      {
        const int64_t o = idx * a.in_sj;
        qf = qp[o];
        dqf = dqp[o];
        ddqf = ddqp[o];
      }
      double s0, s1;
      joint_sincos_state(J.type, qf, s0, s1);
      js.at(TD_S0, f) = s0;
      js.at(TD_S1, f) = s1;
      js.at(TD_DQ, f) = dqf;
      double R[9];
      V3 t;
      joint_transform(J, s0, s1, R, t);
      primal_step(J, R, t, dqf, ddqf, w, vl, al, acc);
      js.put3(TD_W, f, w);
      js.put3(TD_VL, f, vl);
      js.put3(TD_AL, f, al);
      js.put3(TD_AC, f, acc);
      V3 fo, no;
      link_wrench(J, w, vl, al, acc, fo, no);
      js.put3(TD_FC, f, fo);
      js.put3(TD_NC, f, no);
    }
  }
  {
    V3 F = mk(0, 0, 0), N = mk(0, 0, 0);
#pragma unroll 1
    for (int f = nj - 1; f >= 0; --f)
    {
      F = F + js.get3(TD_FC, f);
      N = N + js.get3(TD_NC, f);
      js.put3(TD_FC, f, F);
      js.put3(TD_NC, f, N);
      double R[9];
      V3 t;
      joint_transform(c->j[f], js.at(TD_S0, f), js.at(TD_S1, f), R, t);
      const V3 Fp = rot(R, F);
      N = rot(R, N) + cross(t, Fp);
      F = Fp;
    }
  }
#pragma unroll 1
  for (int kind = 0; kind < 2; ++kind)
  {
    double* const out = kind == 0 ? a.dtau_dq : a.dtau_dv;
    if (!out) continue;
    double* const op = out + s * a.m_ss;
#pragma unroll 1
    for (int k = 0; k < nj; ++k)
    {
      JointRef Jk = c->j[k];
      const int col = Jk.in_idx;
      if (col < 0) continue;
      {
        Tangent d = tangent_seed(kind, Jk.type, ld3(Jk.u), js.get3(TD_W, k), js.get3(TD_VL, k), js.get3(TD_AL, k), js.get3(TD_AC, k));
        V3 dfo, dno;
        tangent_wrench(Jk, js.get3(TD_W, k), js.get3(TD_VL, k), d, dfo, dno);
        js.put3(TD_DF, k, dfo);
        js.put3(TD_DN, k, dno);
#pragma unroll 1
        for (int f = k + 1; f < nj; ++f)
        {
          JointRef J = c->j[f];
          double R[9];
          V3 t;
          joint_transform(J, js.at(TD_S0, f), js.at(TD_S1, f), R, t);
          tangent_step(J, R, t, js.at(TD_DQ, f), d);
          tangent_wrench(J, js.get3(TD_W, f), js.get3(TD_VL, f), d, dfo, dno);
          js.put3(TD_DF, f, dfo);
          js.put3(TD_DN, f, dno);
        }
      }
      V3 dF = mk(0, 0, 0), dN = mk(0, 0, 0);
#pragma unroll 1
      for (int f = nj - 1; f >= 0; --f)
      {
        JointRef J = c->j[f];
        const int type = J.type;
        const V3 u = ld3(J.u);
        if (f >= k)
        {
          dF = dF + js.get3(TD_DF, f);
          dN = dN + js.get3(TD_DN, f);
        }
        const int row = J.in_idx;
        if (row >= 0)
        {
          double v = 0.0;
          if (type == RDYN_REVOLUTE) v = dot(u, dN);
          else if (type == RDYN_PRISMATIC) v = dot(u, dF);
          op[(int64_t)(row + n * col) * a.m_se] = v;
        }
        if (f == 0) break;
        if (kind == 0 && f == k)
        {
          if (type == RDYN_REVOLUTE)
          {
            dF = dF + cross(u, js.get3(TD_FC, k));
            dN = dN + cross(u, js.get3(TD_NC, k));
          }
          else if (type == RDYN_PRISMATIC)
            dN = dN + cross(u, js.get3(TD_FC, k));
        }
        double R[9];
        V3 t;
        joint_transform(J, js.at(TD_S0, f), js.at(TD_S1, f), R, t);
        const V3 Fp = rot(R, dF);
        dN = rot(R, dN) + cross(t, Fp);
        dF = Fp;
      }
    }
  }
}

// LDS one workgroup may ask for on the current device (163 840 bytes on gfx950), asked of the runtime once per device; 0: the query failed
size_t device_lds_limit()
{
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  int v = (dev >= 0 && dev < 64) ? cache[dev].load(std::memory_order_relaxed) : 0;
  if (v > 0) return (size_t)v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) return 0;
  if (dev >= 0 && dev < 64) cache[dev].store(v, std::memory_order_relaxed);
  return (size_t)v;
}

template <int NJ>
hipError_t launch_td_nj(const RdynTorqueDerivArgs& a, hipStream_t st)
{
  const size_t lds = a.staged ? (size_t)64 * (size_t)(a.staged | 1) * 8 : 0;  // <= 51 712 bytes at 10 input joints
  hipLaunchKernelGGL((k_torque_deriv<NJ>), dim3((unsigned)((a.n_samples + 63) / 64)), dim3(64), lds, st, a);
  return hipGetLastError();
}
}  // namespace

hipError_t rdyn_launch_torque_derivatives(int n_joints, const RdynTorqueDerivArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0) return hipSuccess;
#define CALL(N) launch_td_nj<N>(a, st)
  RDYN_DISPATCH_NJ(n_joints, CALL)
#undef CALL
}

size_t rdyn_long_torque_deriv_lds_bytes(int n_joints, int lanes) { return (size_t)TD_VALUES * n_joints * lanes * sizeof(double); }

// lanes (= samples) per workgroup on the current device: the width that keeps most samples resident in the LDS a workgroup may use there,
// the wider one on a tie; 0 = none fits (or the device does not answer)
int rdyn_long_torque_deriv_lanes(int n_joints)
{
  const size_t limit = device_lds_limit();
  int best = 0;
  size_t best_resident = 0;
  for (int lanes = 64; lanes >= 16; lanes /= 2)
  {
    const size_t bytes = rdyn_long_torque_deriv_lds_bytes(n_joints, lanes);
    if (bytes == 0 || bytes > limit) continue;
    const size_t resident = (limit / bytes) * lanes;
    if (resident > best_resident)
    {
      best = lanes;
      best_resident = resident;
    }
  }
  return best;
}

hipError_t rdyn_launch_long_torque_derivatives(int n_joints, const RdynTorqueDerivArgs& a, hipStream_t st)
{
  if (a.n_samples <= 0 || (!a.dtau_dq && !a.dtau_dv)) return hipSuccess;
  const int lanes = rdyn_long_torque_deriv_lanes(n_joints);
  if (lanes == 0) return hipErrorInvalidValue;
  const size_t lds = rdyn_long_torque_deriv_lds_bytes(n_joints, lanes);
  if (lds > 64 * 1024)
  {
    // the device's own limit, not gfx950's 160 KB: the lane count above was chosen for it
    hipError_t e = opt_in_lds_once<k_long_torque_deriv>((int)device_lds_limit());
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_long_torque_deriv, dim3((unsigned)((a.n_samples + lanes - 1) / lanes)), dim3(lanes), lds, st, a);
  return hipGetLastError();
}
