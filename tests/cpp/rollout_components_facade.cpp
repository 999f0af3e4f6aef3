// Forward dynamics and rollouts with components through the C++ facade (rosdyn_chain_facade.hpp): getJointAccelerationBatch and
// rolloutBatch with a leading component list, and the single-sample getJointAcceleration(q, Dq, tau, comps), on inputs that are exact
// binary fractions; prints every result with 17 digits for tests/test_gpu_rollout_components.py to compare with the Python binding's.
// usage: prog chain.urdf base tool
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

static double value(int s, int i, int k) { return ((s * 7 + i * 3 + k * 5) % 17 - 8) / 16.0; }

static void print(const char* what, const std::vector<double>& v)
{
  std::printf("%s", what);
  for (double x : v) std::printf(" %.17g", x);
  std::printf("\n");
}

static void run(const char* urdf, const char* base, const char* tool)
{
  rosdyn::ChainPtr chain = rosdyn::createChain(slurp(urdf), base, tool, {0.0, 0.0, -9.806});
  const int n = (int)chain->getActiveJointsNumber();
  const int N = 5, T = 3;
  std::vector<rdyn_component> comps(3);
  std::memset(comps.data(), 0, comps.size() * sizeof(rdyn_component));
  comps[0].type = RDYN_COMP_FRICTION1; comps[0].joint = 0; comps[0].min_velocity = 0.0625; comps[0].max_velocity = 0.75;
  comps[0].parameters[0] = 0.25; comps[0].parameters[1] = 0.5;
  comps[1].type = RDYN_COMP_FRICTION2; comps[1].joint = n - 1; comps[1].min_velocity = 0.0625; comps[1].max_velocity = 0.75;
  comps[1].parameters[0] = 0.125; comps[1].parameters[1] = 0.25; comps[1].parameters[2] = -0.5;
  comps[2].type = RDYN_COMP_SPRING; comps[2].joint = 0; comps[2].parameters[0] = 1.5; comps[2].parameters[1] = -0.25;
  const size_t cnt = (size_t)N * n, bytes = cnt * sizeof(double);
  std::vector<double> hq(cnt), hdq(cnt), htau(cnt * T), out(cnt);
  for (int s = 0; s < N; ++s)
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      for (int t = 0; t < T; ++t) htau[t * cnt + (size_t)s * n + i] = 0.5 * value(s, i, 2 + t);
    }
  double *d_q = nullptr, *d_dq = nullptr, *d_tau = nullptr, *d_ddq = nullptr, *d_qe = nullptr, *d_dqe = nullptr;
  int32_t* d_st = nullptr;
  void* ws = nullptr;
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
  d.integrator = RDYN_INTEGRATOR_RK4;
  d.dt = 1e-3;
  d.tau = d_tau;
  d.tau_step_stride = (int64_t)cnt;
  d.q_end = d_qe;
  d.dq_end = d_dqe;
  d.status = d_st;
  const size_t ws_bytes = chain->rolloutWorkspaceBytes(d, N, 0);   // covers the forward dynamics' workspace too
  if (ws_bytes) HIP_OK(hipMalloc(&ws, ws_bytes));
  std::vector<int32_t> hst(N);
  chain->getJointAccelerationBatch(comps, b, d_tau, d_ddq, d_st, 0, ws, ws_bytes);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out.data(), d_ddq, bytes, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(hst.data(), d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < N; ++s)
    if (hst[s] != 1) throw std::runtime_error("forward dynamics status");
  print("ddq", out);
  chain->rolloutBatch(comps, b, d, 0, ws, ws_bytes);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(hst.data(), d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int s = 0; s < N; ++s)
    if (hst[s] != 1) throw std::runtime_error("rollout status");
  HIP_OK(hipMemcpy(out.data(), d_qe, bytes, hipMemcpyDeviceToHost));
  print("q_end", out);
  HIP_OK(hipMemcpy(out.data(), d_dqe, bytes, hipMemcpyDeviceToHost));
  print("dq_end", out);
  // the single-sample getter on sample 0
  rosdyn::VectorXd q(n), Dq(n), tau(n);
  for (int i = 0; i < n; ++i)
  {
    q(i) = hq[i];
    Dq(i) = hdq[i];
    tau(i) = htau[i];
  }
  const rosdyn::VectorXd one = chain->getJointAcceleration(q, Dq, tau, comps);
  std::vector<double> first(n);
  for (int i = 0; i < n; ++i) first[i] = one(i);
  print("single", first);
  // an invalid list throws what the batch methods throw for invalid arguments
  comps[1].joint = n;
  bool threw = false;
  try
  {
    chain->rolloutBatch(comps, b, d, 0, ws, ws_bytes);
  }
  catch (const std::invalid_argument&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception on a component joint out of range");
  (void)hipFree(d_q);
  (void)hipFree(d_dq);
  (void)hipFree(d_tau);
  (void)hipFree(d_ddq);
  (void)hipFree(d_qe);
  (void)hipFree(d_dqe);
  (void)hipFree(d_st);
  if (ws) (void)hipFree(ws);
}

int main(int argc, char** argv)
{
  if (argc < 4)
  {
    std::fprintf(stderr, "usage: %s chain.urdf base tool\n", argv[0]);
    return 2;
  }
  try
  {
    run(argv[1], argv[2], argv[3]);
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
