// Rollouts through the C++ facade (rosdyn_chain_facade.hpp): rolloutBatch on a chain swept in registers (ur10_like, 6 joints) and on one
// with 14 input joints (the chunked route) against semi-implicit Euler steps chained on the host over getJointAccelerationBatch; the
// exception on an invalid descriptor.  usage: prog ur10_like.urdf rev14.urdf
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
  const int N = 300, T = 5;
  const double dt = 1e-3;
  const size_t cnt = (size_t)N * n, bytes = cnt * sizeof(double);
  std::vector<double> hq(cnt), hdq(cnt), htau(cnt * T), hddq(cnt);
  for (int s = 0; s < N; ++s)
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      for (int t = 0; t < T; ++t) htau[t * cnt + (size_t)s * n + i] = 0.4 * value(s, i, 2 + t);
    }
  double *d_q = nullptr, *d_dq = nullptr, *d_tau = nullptr, *d_ddq = nullptr, *d_qe = nullptr, *d_dqe = nullptr;
  int32_t* d_st = nullptr;
  void *ws = nullptr, *fws = nullptr;
  HIP_OK(hipMalloc((void**)&d_q, bytes));
  HIP_OK(hipMalloc((void**)&d_dq, bytes));
  HIP_OK(hipMalloc((void**)&d_tau, bytes * T));
  HIP_OK(hipMalloc((void**)&d_ddq, bytes));
  HIP_OK(hipMalloc((void**)&d_qe, bytes));
  HIP_OK(hipMalloc((void**)&d_dqe, bytes));
  HIP_OK(hipMalloc((void**)&d_st, N * sizeof(int32_t)));
  HIP_OK(hipMemcpy(d_q, hq.data(), bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_dq, hdq.data(), bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_tau, htau.data(), bytes * T, hipMemcpyHostToDevice));
  rdyn_batch b;
  std::memset(&b, 0, sizeof b);
  b.n_samples = N;
  b.q = d_q;
  b.dq = d_dq;
  b.layout = RDYN_LAYOUT_SAMPLE_MAJOR;
  b.device = -1;
  rdyn_rollout_desc d;
  std::memset(&d, 0, sizeof d);
  d.n_steps = T;
  d.integrator = RDYN_INTEGRATOR_SEMI_IMPLICIT_EULER;
  d.dt = dt;
  d.tau = d_tau;
  d.tau_step_stride = (int64_t)cnt;
  d.q_end = d_qe;
  d.dq_end = d_dqe;
  d.status = d_st;
  const size_t ws_bytes = chain->rolloutWorkspaceBytes(d, N, 128);
  if ((n > 10) != (ws_bytes > 0)) throw std::runtime_error("workspace query");
  if (ws_bytes) HIP_OK(hipMalloc(&ws, ws_bytes));
  chain->rolloutBatch(b, d, 128, ws, ws_bytes);
  HIP_OK(hipDeviceSynchronize());
  std::vector<double> q_end(cnt), dq_end(cnt);
  std::vector<int32_t> hst(N);
  HIP_OK(hipMemcpy(q_end.data(), d_qe, bytes, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(dq_end.data(), d_dqe, bytes, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hst.data(), d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < N; ++s)
    if (hst[s] != 1) throw std::runtime_error("rollout status");
  // ---- the same steps chained on the host over getJointAccelerationBatch
  const size_t fws_bytes = chain->getJointAccelerationWorkspaceBytes(128);
  if (fws_bytes) HIP_OK(hipMalloc(&fws, fws_bytes));
  double amax = 0.0;
  for (int t = 0; t < T; ++t)
  {
    HIP_OK(hipMemcpy(d_q, hq.data(), bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_dq, hdq.data(), bytes, hipMemcpyHostToDevice));
    chain->getJointAccelerationBatch(b, d_tau + t * cnt, d_ddq, d_st, 128, fws, fws_bytes);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(hddq.data(), d_ddq, bytes, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < cnt; ++e)
    {
      amax = std::fmax(amax, std::fabs(hddq[e]));
      hdq[e] = hdq[e] + dt * hddq[e];
      hq[e] = hq[e] + dt * hdq[e];
    }
  }
  // same kernels' arithmetic at states that differ by roundings of the update (fused on the device): a loose parity figure suffices here,
  // the sharp bounds are in tests/test_gpu_rollout.py
  for (size_t e = 0; e < cnt; ++e)
  {
    if (!(std::fabs(q_end[e] - hq[e]) <= 1e-10 * std::fmax(1.0, amax))) throw std::runtime_error("q_end != chained steps");
    if (!(std::fabs(dq_end[e] - hdq[e]) <= 1e-10 * std::fmax(1.0, amax))) throw std::runtime_error("dq_end != chained steps");
  }
  // ---- an invalid descriptor throws what the batch methods throw for invalid arguments
  d.dt = 0.0;
  bool threw = false;
  try
  {
    chain->rolloutBatch(b, d, 128, ws, ws_bytes);
  }
  catch (const std::invalid_argument&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception on dt = 0");
  (void)hipFree(d_q);
  (void)hipFree(d_dq);
  (void)hipFree(d_tau);
  (void)hipFree(d_ddq);
  (void)hipFree(d_qe);
  (void)hipFree(d_dqe);
  (void)hipFree(d_st);
  if (ws) (void)hipFree(ws);
  if (fws) (void)hipFree(fws);
}

int main(int argc, char** argv)
{
  if (argc < 3)
  {
    std::fprintf(stderr, "usage: %s ur10_like.urdf rev14.urdf\n", argv[0]);
    return 2;
  }
  try
  {
    check_chain(argv[1], "base_link", "tool0");
    check_chain(argv[2], "l0", "l14");
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
