// Forward dynamics through the C++ facade (rosdyn_chain_facade.hpp): the single-sample getter getJointAcceleration and the batch method
// getJointAccelerationBatch, on a chain swept in registers (ur10_like, 6 joints) and on one with 14 input joints (the chunked route);
// the exception on an inertia matrix that is not positive definite.  usage: prog ur10_like.urdf ur10_public.urdf rev14.urdf
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

static double value(int s, int i, int k) { return std::sin(0.37 * (s + 1) + 1.3 * i + 2.1 * k); }

static void check_chain(const char* urdf, const char* base, const char* tool)
{
  rosdyn::ChainPtr chain = rosdyn::createChain(slurp(urdf), base, tool, {0.0, 0.0, -9.806});
  const int n = (int)chain->getActiveJointsNumber();
  const int N = 300;
  std::vector<double> hq((size_t)N * n), hdq(hq.size()), htau(hq.size()), hddq(hq.size());
  for (int s = 0; s < N; ++s)
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      htau[(size_t)s * n + i] = 50.0 * value(s, i, 2);
    }
  // ---- the batch method
  double *dq_q = nullptr, *dq_dq = nullptr, *d_tau = nullptr, *d_ddq = nullptr;
  int32_t* d_st = nullptr;
  void* ws = nullptr;
  const size_t bytes = hq.size() * sizeof(double);
  HIP_OK(hipMalloc((void**)&dq_q, bytes));
  HIP_OK(hipMalloc((void**)&dq_dq, bytes));
  HIP_OK(hipMalloc((void**)&d_tau, bytes));
  HIP_OK(hipMalloc((void**)&d_ddq, bytes));
  HIP_OK(hipMalloc((void**)&d_st, N * sizeof(int32_t)));
  const size_t ws_bytes = chain->getJointAccelerationWorkspaceBytes(128);
  if ((n > 10) != (ws_bytes > 0)) throw std::runtime_error("workspace query");
  if (ws_bytes) HIP_OK(hipMalloc(&ws, ws_bytes));
  HIP_OK(hipMemcpy(dq_q, hq.data(), bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dq_dq, hdq.data(), bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_tau, htau.data(), bytes, hipMemcpyHostToDevice));
  rdyn_batch b;
  std::memset(&b, 0, sizeof b);
  b.n_samples = N;
  b.q = dq_q;
  b.dq = dq_dq;
  b.layout = RDYN_LAYOUT_SAMPLE_MAJOR;
  b.device = -1;
  chain->getJointAccelerationBatch(b, d_tau, d_ddq, d_st, 128, ws, ws_bytes);
  HIP_OK(hipDeviceSynchronize());
  std::vector<int32_t> hst(N);
  HIP_OK(hipMemcpy(hddq.data(), d_ddq, bytes, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hst.data(), d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < N; ++s)
    if (hst[s] != 1) throw std::runtime_error("batch status");
  // ---- the single-sample getter on three of the samples: equal to the batch, and M ddq + h = tau with the facade's own M and h
  const int picks[3] = {0, 137, N - 1};
  for (int p = 0; p < 3; ++p)
  {
    const int s = picks[p];
    rosdyn::VectorXd q(n), dq(n), tau(n);
    for (int i = 0; i < n; ++i)
    {
      q(i) = hq[(size_t)s * n + i];
      dq(i) = hdq[(size_t)s * n + i];
      tau(i) = htau[(size_t)s * n + i];
    }
    const rosdyn::VectorXd ddq = chain->getJointAcceleration(q, dq, tau);
    if (ddq.rows() != n) throw std::runtime_error("single: size");
    const rosdyn::MatrixXd M = chain->getJointInertia(q);
    const rosdyn::VectorXd h = chain->getJointTorqueNonLinearPart(q, dq);
    double scale = 0.0, worst = 0.0, amax = 0.0;
    for (int i = 0; i < n; ++i) amax = std::fmax(amax, std::fabs(ddq(i)));
    for (int i = 0; i < n; ++i)
    {
      double r = h(i) - tau(i), row = 0.0;
      for (int j = 0; j < n; ++j)
      {
        r += M(i, j) * ddq(j);
        row += std::fabs(M(i, j));
      }
      worst = std::fmax(worst, std::fabs(r));
      scale = std::fmax(scale, row * amax + std::fabs(tau(i)) + std::fabs(h(i)));
      if (std::fabs(ddq(i) - hddq[(size_t)s * n + i]) > 1e-12 * std::fmax(1.0, amax)) throw std::runtime_error("single != batch");
    }
    if (!(worst <= 1e-11 * scale)) throw std::runtime_error("single: residual");
  }
  (void)hipFree(dq_q);
  (void)hipFree(dq_dq);
  (void)hipFree(d_tau);
  (void)hipFree(d_ddq);
  (void)hipFree(d_st);
  if (ws) (void)hipFree(ws);
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
    check_chain(argv[1], "base_link", "tool0");
    check_chain(argv[3], "l0", "l14");
    // a fixed joint among the input joints: its row of M is zero -> status -1 -> the getter throws
    rosdyn::ChainPtr bad = rosdyn::createChain(slurp(argv[2]), "base_link", "tool0", {0.0, 0.0, -9.806});
    if (!bad->setInputJointsName({"shoulder_pan_joint", "shoulder_lift_joint", "flange-tool0", "elbow_joint"})) throw std::runtime_error("setInputJointsName");
    rosdyn::VectorXd q(4), dq(4), tau(4);
    for (int i = 0; i < 4; ++i) q(i) = dq(i) = tau(i) = 0.1 * (i + 1);
    bool threw = false;
    try
    {
      (void)bad->getJointAcceleration(q, dq, tau);
    }
    catch (const std::runtime_error&)
    {
      threw = true;
    }
    if (!threw) throw std::runtime_error("no exception on a singular inertia matrix");
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
