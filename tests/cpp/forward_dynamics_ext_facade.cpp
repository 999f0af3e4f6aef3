// Forward dynamics and rollouts with external link wrenches through the C++ facade (rosdyn_chain_facade.hpp): getJointAccelerationBatch and
// rolloutBatch with a rdyn_ext_wrenches (every link, then the tool alone with a per-step sequence), and the single-sample
// getJointAcceleration(q, Dq, tau, ext_wrenches_in_link_frame), on inputs that are exact binary fractions; prints every result with 17
// digits for tests/test_forward_dynamics_ext_facade.py to compare with the Python binding's.
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

template <class T>
static T* device_copy(const std::vector<T>& h)
{
  T* d = nullptr;
  HIP_OK(hipMalloc((void**)&d, h.size() * sizeof(T)));
  HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

static void run(const char* urdf, const char* base, const char* tool)
{
  rosdyn::ChainPtr chain = rosdyn::createChain(slurp(urdf), base, tool, {0.0, 0.0, -9.806});
  const int n = (int)chain->getActiveJointsNumber(), L = (int)chain->getLinksNumber();
  const int N = 5, T = 3;
  const size_t cnt = (size_t)N * n, bytes = cnt * sizeof(double);
  std::vector<double> hq(cnt), hdq(cnt), htau(cnt * T), hall((size_t)N * L * 6), htool((size_t)T * N * 6), out(cnt);
  for (int s = 0; s < N; ++s)
  {
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      for (int t = 0; t < T; ++t) htau[t * cnt + (size_t)s * n + i] = 0.5 * value(s, i, 2 + t);
    }
    for (int e = 0; e < 6 * L; ++e) hall[(size_t)s * 6 * L + e] = 0.25 * value(s, e, 11);
    for (int t = 0; t < T; ++t)
      for (int e = 0; e < 6; ++e) htool[((size_t)t * N + s) * 6 + e] = 0.5 * value(s, e, 12 + t);
  }
  double *d_q = device_copy(hq), *d_dq = device_copy(hdq), *d_tau = device_copy(htau), *d_all = device_copy(hall), *d_tool = device_copy(htool);
  double *d_ddq = nullptr, *d_qe = nullptr, *d_dqe = nullptr;
  int32_t* d_st = nullptr;
  void* ws = nullptr;
  HIP_OK(hipMalloc((void**)&d_ddq, bytes));
  HIP_OK(hipMalloc((void**)&d_qe, bytes));
  HIP_OK(hipMalloc((void**)&d_dqe, bytes));
  HIP_OK(hipMalloc((void**)&d_st, N * sizeof(int32_t)));
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
  const rdyn_ext_wrenches all = {d_all, -1, 0};
  const rdyn_ext_wrenches tool_seq = {d_tool, (int32_t)chain->getJointsNumber(), (int64_t)N * 6};
  const std::vector<rdyn_component> none;
  const size_t ws_bytes = chain->rolloutWorkspaceBytes(d, all, N, 0);   // covers the forward dynamics' workspace too
  if (ws_bytes < chain->getJointAccelerationWorkspaceBytes(all, 0)) throw std::runtime_error("workspace queries");
  if (ws_bytes) HIP_OK(hipMalloc(&ws, ws_bytes));
  std::vector<int32_t> hst(N);
  auto status_ok = [&](const char* what) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(hst.data(), d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int s = 0; s < N; ++s)
      if (hst[s] != 1) throw std::runtime_error(what);
  };
  auto fetch = [&](const char* what, const double* dev) {
    HIP_OK(hipMemcpy(out.data(), dev, bytes, hipMemcpyDeviceToHost));
    print(what, out);
  };
  chain->getJointAccelerationBatch(none, all, b, d_tau, d_ddq, d_st, 0, ws, ws_bytes);
  status_ok("forward dynamics status");
  fetch("ddq", d_ddq);
  chain->rolloutBatch(none, all, b, d, 0, ws, ws_bytes);
  status_ok("rollout status");
  fetch("q_end", d_qe);
  fetch("dq_end", d_dqe);
  chain->rolloutBatch(none, tool_seq, b, d, 0, ws, ws_bytes);
  status_ok("rollout status, tool sequence");
  fetch("q_end_tool", d_qe);
  fetch("dq_end_tool", d_dqe);
  // the single-sample getter on sample 0
  rosdyn::VectorXd q(n), Dq(n), tau(n);
  for (int i = 0; i < n; ++i)
  {
    q(i) = hq[i];
    Dq(i) = hdq[i];
    tau(i) = htau[i];
  }
  rosdyn::VectorOfVector6d ext((size_t)L);
  for (int l = 0; l < L; ++l)
    for (int e = 0; e < 6; ++e) ext[(size_t)l](e) = hall[(size_t)6 * l + e];
  const rosdyn::VectorXd one = chain->getJointAcceleration(q, Dq, tau, ext);
  std::vector<double> first(n);
  for (int i = 0; i < n; ++i) first[i] = one(i);
  print("single", first);
  // a link outside the chain throws what the batch methods throw for invalid arguments; so does a wrench list of the wrong length
  bool threw = false;
  try
  {
    const rdyn_ext_wrenches bad = {d_tool, (int32_t)chain->getJointsNumber() + 1, 0};
    chain->rolloutBatch(none, bad, b, d, 0, ws, ws_bytes);
  }
  catch (const std::invalid_argument&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception on a wrench link out of range");
  threw = false;
  try
  {
    ext.pop_back();
    (void)chain->getJointAcceleration(q, Dq, tau, ext);
  }
  catch (const std::invalid_argument&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception on a wrench list of the wrong length");
  (void)hipFree(d_q);
  (void)hipFree(d_dq);
  (void)hipFree(d_tau);
  (void)hipFree(d_all);
  (void)hipFree(d_tool);
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
