// Derivatives of the forward dynamics through the C++ facade (rosdyn_chain_facade.hpp): the batch method
// getJointAccelerationDerivativesBatch and the single-sample getter getJointAccelerationDerivatives, on a chain swept in registers
// (ur10_like, 6 joints), on one with input joints out of chain order (ur10_public, 4 of 6) and on one with 14 input joints (the chunked
// route), each without and with friction and spring components.
// usage: prog ur10_like.urdf ur10_public.urdf rev14.urdf
// Checks: single sample == batch (the same kernels: the same bits); ddq == getJointAcceleration; getJointInertia x dDDq_dtau = 1 to 1e-9;
// every column against a central difference of the facade's own getJointAcceleration with step h = 1e-5 on samples whose velocities keep
// 1e-3 away from the kinks of the friction components: truncation h^2 / 6 |FD'''| ~ 2e-11 |FD'''|, rounding eps cond(M) |ddq| / h -- bound
// 1e-6 (max|D| + |ddq|_inf): a wrong term shows at order 1.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "rosdyn_chain_facade.hpp"

static std::string slurp(const char* path)
{
  std::ifstream f(path);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

#define HIP_OK(x)                                                     \
  do                                                                  \
  {                                                                   \
    if ((x) != hipSuccess) throw std::runtime_error("HIP: " #x);      \
  } while (0)

static const double kMinVelocity = 0.3, kMaxVelocity = 0.8;

static double value(int s, int i, int k) { return std::sin(0.37 * (s + 1) + 1.3 * i + 2.1 * k); }

static bool near_a_kink(double v)
{
  const double a = std::fabs(v);
  return std::fabs(a - kMinVelocity) < 1e-3 || std::fabs(a - kMaxVelocity) < 1e-3;
}

static void check_chain(rosdyn::ChainPtr chain, bool with_components)
{
  const int n = (int)chain->getActiveJointsNumber();
  const int N = 300;
  const size_t nn = (size_t)n * n;
  std::vector<rdyn_component> comps;
  if (with_components)
  {
    rdyn_component c;
    std::memset(&c, 0, sizeof c);
    c.type = RDYN_COMP_FRICTION1;
    c.joint = 0;
    c.min_velocity = kMinVelocity;
    c.max_velocity = kMaxVelocity;
    c.parameters[0] = 2.0;
    c.parameters[1] = 1.5;
    comps.push_back(c);
    c.type = RDYN_COMP_FRICTION2;
    c.joint = n - 1;
    c.parameters[0] = 1.0;
    c.parameters[1] = 0.8;
    c.parameters[2] = -0.6;
    comps.push_back(c);
    c.type = RDYN_COMP_SPRING;
    c.joint = 0;
    c.parameters[0] = -1.5;
    c.parameters[1] = 0.3;
    c.parameters[2] = 0.0;
    comps.push_back(c);
  }
  std::vector<double> hq((size_t)N * n), hdq(hq.size()), htau(hq.size());
  for (int s = 0; s < N; ++s)
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      htau[(size_t)s * n + i] = 20.0 * value(s, i, 2);
    }
  // ---- the batch method
  double *d_q = nullptr, *d_dq = nullptr, *d_tau = nullptr, *d_ddq = nullptr, *d_out = nullptr;
  int32_t* d_st = nullptr;
  void* d_ws = nullptr;
  const size_t bytes = hq.size() * sizeof(double), obytes = (size_t)N * nn * sizeof(double);
  const size_t ws_bytes = chain->getJointAccelerationDerivativesWorkspaceBytes(128);
  if ((n > 10) != (ws_bytes > 0)) throw std::runtime_error("workspace query");
  HIP_OK(hipMalloc((void**)&d_q, bytes));
  HIP_OK(hipMalloc((void**)&d_dq, bytes));
  HIP_OK(hipMalloc((void**)&d_tau, bytes));
  HIP_OK(hipMalloc((void**)&d_ddq, bytes));
  HIP_OK(hipMalloc((void**)&d_out, 3 * obytes));
  HIP_OK(hipMalloc((void**)&d_st, N * sizeof(int32_t)));
  if (ws_bytes) HIP_OK(hipMalloc(&d_ws, ws_bytes));
  HIP_OK(hipMemcpy(d_q, hq.data(), bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_dq, hdq.data(), bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_tau, htau.data(), bytes, hipMemcpyHostToDevice));
  rdyn_batch b;
  std::memset(&b, 0, sizeof b);
  b.n_samples = N;
  b.q = d_q;
  b.dq = d_dq;
  b.layout = RDYN_LAYOUT_SAMPLE_MAJOR;
  b.device = -1;
  chain->getJointAccelerationDerivativesBatch(comps, b, d_tau, d_ddq, d_out, d_out + (size_t)N * nn, d_out + 2 * (size_t)N * nn, d_st, 128, d_ws,
                                              ws_bytes);
  HIP_OK(hipDeviceSynchronize());
  std::vector<double> hout(3 * (size_t)N * nn), hddq(hq.size());
  std::vector<int32_t> hst(N);
  HIP_OK(hipMemcpy(hout.data(), d_out, 3 * obytes, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hddq.data(), d_ddq, bytes, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hst.data(), d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < N; ++s)
    if (hst[s] != 1) throw std::runtime_error("batch status");
  const double* const bmat[3] = {hout.data(), hout.data() + (size_t)N * nn, hout.data() + 2 * (size_t)N * nn};
  // ---- the single-sample getter on three samples that keep away from the kinks
  const double h = 1e-5;
  int checked = 0;
  for (int s = 0; s < N && checked < 3; s += 37)
  {
    bool skip = false;
    for (int i = 0; i < n; ++i) skip = skip || near_a_kink(hdq[(size_t)s * n + i]);
    if (skip) continue;
    ++checked;
    rosdyn::VectorXd q(n), dq(n), tau(n);
    for (int i = 0; i < n; ++i)
    {
      q(i) = hq[(size_t)s * n + i];
      dq(i) = hdq[(size_t)s * n + i];
      tau(i) = htau[(size_t)s * n + i];
    }
    rosdyn::MatrixXd D[3];
    const rosdyn::VectorXd ddq = with_components ? chain->getJointAccelerationDerivatives(q, dq, tau, comps, D[0], D[1], D[2])
                                                 : chain->getJointAccelerationDerivatives(q, dq, tau, D[0], D[1], D[2]);
    const rosdyn::VectorXd ddq0 = with_components ? chain->getJointAcceleration(q, dq, tau, comps) : chain->getJointAcceleration(q, dq, tau);
    double scale = 0.0;
    for (int i = 0; i < n; ++i)
    {
      if (ddq(i) != ddq0(i) || ddq(i) != hddq[(size_t)s * n + i]) throw std::runtime_error("ddq: single, batch and getJointAcceleration differ");
      scale = std::fmax(scale, std::fabs(ddq(i)));
    }
    double dmax = 0.0;
    for (int m = 0; m < 3; ++m)
    {
      if (D[m].rows() != n || D[m].cols() != n) throw std::runtime_error("single: size");
      for (int k = 0; k < n; ++k)
        for (int i = 0; i < n; ++i)
        {
          if (D[m](i, k) != bmat[m][(size_t)s * nn + (size_t)i + (size_t)n * k]) throw std::runtime_error("single != batch");
          dmax = std::fmax(dmax, std::fabs(D[m](i, k)));
        }
    }
    scale += dmax;
    const rosdyn::MatrixXd M = chain->getJointInertia(q);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < n; ++k)
      {
        double acc = 0.0, mag = 0.0;
        for (int j = 0; j < n; ++j)
        {
          acc += M(i, j) * D[2](j, k);
          mag += std::fabs(M(i, j) * D[2](j, k));
        }
        if (!(std::fabs(acc - (i == k ? 1.0 : 0.0)) <= 1e-9 * (mag + 1.0))) throw std::runtime_error("getJointInertia x dDDq_dtau is not the identity");
      }
    for (int k = 0; k < n; ++k)
      for (int which = 0; which < 3; ++which)
      {
        rosdyn::VectorXd xp = which == 0 ? q : (which == 1 ? dq : tau), xm = xp;
        xp(k) += h;
        xm(k) -= h;
        auto fd_at = [&](const rosdyn::VectorXd& x) {
          const rosdyn::VectorXd& a = which == 0 ? x : q;
          const rosdyn::VectorXd& v = which == 1 ? x : dq;
          const rosdyn::VectorXd& t = which == 2 ? x : tau;
          return with_components ? chain->getJointAcceleration(a, v, t, comps) : chain->getJointAcceleration(a, v, t);
        };
        const rosdyn::VectorXd ap = fd_at(xp), am = fd_at(xm);
        for (int i = 0; i < n; ++i)
        {
          const double fd = (ap(i) - am(i)) / (2.0 * h);
          const double got = D[which](i, k);
          if (!(std::fabs(fd - got) <= 1e-6 * scale))
          {
            std::fprintf(stderr, "sample %d matrix %d (%d, %d): %.12g against the central difference %.12g (scale %.3g)\n", s, which, i, k, got, fd,
                         scale);
            throw std::runtime_error("derivative against the central difference");
          }
        }
      }
  }
  if (checked < 3) throw std::runtime_error("fewer than three samples away from the kinks");
  // every matrix null is refused
  bool threw = false;
  try
  {
    chain->getJointAccelerationDerivativesBatch(comps, b, d_tau, d_ddq, nullptr, nullptr, nullptr, d_st, 128, d_ws, ws_bytes);
  }
  catch (const std::exception&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception when every matrix is null");
  (void)hipFree(d_q);
  (void)hipFree(d_dq);
  (void)hipFree(d_tau);
  (void)hipFree(d_ddq);
  (void)hipFree(d_out);
  (void)hipFree(d_st);
  if (d_ws) (void)hipFree(d_ws);
}

int main(int argc, char** argv)
{
  if (argc < 4)
  {
    std::fprintf(stderr, "usage: %s ur10_like.urdf ur10_public.urdf rev14.urdf\n", argv[0]);
    return 2;
  }
  try
  {
    for (int with_components = 0; with_components < 2; ++with_components)
    {
      check_chain(rosdyn::createChain(slurp(argv[1]), "base_link", "tool0", {0.0, 0.0, -9.806}), with_components != 0);
      rosdyn::ChainPtr perm = rosdyn::createChain(slurp(argv[2]), "base_link", "tool0", {0.0, 0.0, -9.806});
      if (!perm->setInputJointsName({"wrist_1_joint", "shoulder_pan_joint", "elbow_joint", "shoulder_lift_joint"})) throw std::runtime_error("setInputJointsName");
      check_chain(perm, with_components != 0);
      check_chain(rosdyn::createChain(slurp(argv[3]), "l0", "l14", {0.0, 0.0, -9.806}), with_components != 0);
    }
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
