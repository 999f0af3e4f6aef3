// Reverse mode through external link wrenches through the C++ facade (rosdyn_chain_facade.hpp): getJointAccelerationVjpBatch and
// rolloutAdjointBatch with a rdyn_ext_wrenches (every link with the summed wrench gradient, then the tool alone with a per-step sequence
// and a gradient per step), on inputs that are exact binary fractions; prints every result with 17 digits for
// tests/test_rollout_adjoint_ext_facade.py to compare with the Python binding's.
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
  const size_t cnt = (size_t)N * n;
  std::vector<double> hq(cnt), hdq(cnt), htau(cnt * T), hseed(cnt), hall((size_t)N * L * 6), htool((size_t)T * N * 6);
  for (int s = 0; s < N; ++s)
  {
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      hseed[(size_t)s * n + i] = value(s, i, 9);
      for (int t = 0; t < T; ++t) htau[t * cnt + (size_t)s * n + i] = 0.5 * value(s, i, 2 + t);
    }
    for (int e = 0; e < 6 * L; ++e) hall[(size_t)s * 6 * L + e] = 0.25 * value(s, e, 11);
    for (int t = 0; t < T; ++t)
      for (int e = 0; e < 6; ++e) htool[((size_t)t * N + s) * 6 + e] = 0.5 * value(s, e, 12 + t);
  }
  double *d_q = device_copy(hq), *d_dq = device_copy(hdq), *d_tau = device_copy(htau), *d_seed = device_copy(hseed), *d_all = device_copy(hall),
         *d_tool = device_copy(htool);
  // n-vectors per sample: q_bar / gq0 | dq_bar / gdq0 | tau_bar | ddq | the end state of the forward call (2)
  std::vector<double*> d_vec(6);
  for (double*& p : d_vec) HIP_OK(hipMalloc((void**)&p, cnt * sizeof(double)));
  double *d_eall = nullptr, *d_etool = nullptr;
  HIP_OK(hipMalloc((void**)&d_eall, hall.size() * sizeof(double)));
  HIP_OK(hipMalloc((void**)&d_etool, htool.size() * sizeof(double)));
  int32_t* d_st = nullptr;
  HIP_OK(hipMalloc((void**)&d_st, N * sizeof(int32_t)));
  rdyn_batch b;
  std::memset(&b, 0, sizeof b);
  b.n_samples = N;
  b.q = d_q;
  b.dq = d_dq;
  b.layout = RDYN_LAYOUT_SAMPLE_MAJOR;
  b.device = -1;
  const rdyn_ext_wrenches all = {d_all, -1, 0};
  const rdyn_ext_wrenches tool_seq = {d_tool, (int32_t)chain->getJointsNumber(), (int64_t)N * 6};
  const std::vector<rdyn_component> none;
  std::vector<int32_t> hst(N);
  auto status_ok = [&](const char* what) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(hst.data(), d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int s = 0; s < N; ++s)
      if (hst[s] != 1) throw std::runtime_error(what);
  };
  auto fetch = [&](const char* what, const double* dev, size_t count) {
    std::vector<double> out(count);
    HIP_OK(hipMemcpy(out.data(), dev, count * sizeof(double), hipMemcpyDeviceToHost));
    print(what, out);
  };
  // the product, every link
  if (chain->getJointAccelerationVjpWorkspaceBytes(all, 0) != 0) throw std::runtime_error("the product with wrenches needs no workspace");
  chain->getJointAccelerationVjpBatch(none, all, b, d_tau, d_seed, d_vec[0], d_vec[1], d_vec[2], d_eall, d_vec[3], d_st, 0, nullptr, 0);
  status_ok("product status");
  fetch("q_bar", d_vec[0], cnt);
  fetch("dq_bar", d_vec[1], cnt);
  fetch("tau_bar", d_vec[2], cnt);
  fetch("ext_bar", d_eall, hall.size());
  fetch("ddq", d_vec[3], cnt);
  // the adjoint: the forward rollout first, for its trajectory with one record per step
  double *d_qt = nullptr, *d_dqt = nullptr;
  HIP_OK(hipMalloc((void**)&d_qt, (size_t)T * cnt * sizeof(double)));
  HIP_OK(hipMalloc((void**)&d_dqt, (size_t)T * cnt * sizeof(double)));
  for (int mode = 0; mode < 2; ++mode)
  {
    const rdyn_ext_wrenches& x = mode ? tool_seq : all;
    rdyn_rollout_desc f;
    std::memset(&f, 0, sizeof f);
    f.n_steps = T;
    f.integrator = RDYN_INTEGRATOR_RK4;
    f.dt = 1e-3;
    f.tau = d_tau;
    f.tau_step_stride = (int64_t)cnt;
    f.q_end = d_vec[4];
    f.dq_end = d_vec[5];
    f.status = d_st;
    f.q_traj = d_qt;
    f.dq_traj = d_dqt;
    f.traj_step_stride = (int64_t)cnt;
    f.traj_every = 1;
    if (chain->rolloutWorkspaceBytes(f, x, N, 0) != 0) throw std::runtime_error("a swept chain needs no workspace");
    chain->rolloutBatch(none, x, b, f, 0, nullptr, 0);
    status_ok("rollout status");
    double* d_gtau = nullptr;
    HIP_OK(hipMalloc((void**)&d_gtau, (size_t)T * cnt * sizeof(double)));
    rdyn_rollout_adjoint_desc a;
    std::memset(&a, 0, sizeof a);
    a.n_steps = T;
    a.integrator = RDYN_INTEGRATOR_RK4;
    a.dt = 1e-3;
    a.tau = d_tau;
    a.tau_step_stride = (int64_t)cnt;
    a.q_traj = d_qt;
    a.dq_traj = d_dqt;
    a.traj_step_stride = (int64_t)cnt;
    a.gq_end = d_seed;
    a.gq0 = d_vec[0];
    a.gdq0 = d_vec[1];
    a.gtau = d_gtau;
    a.gtau_step_stride = (int64_t)cnt;
    a.status = d_st;
    const rdyn_ext_wrench_gradient g = {mode ? d_etool : d_eall, mode ? (int64_t)N * 6 : 0};
    if (chain->rolloutAdjointWorkspaceBytes(a, x, N, 0) != 0) throw std::runtime_error("the adjoint with wrenches needs no workspace");
    chain->rolloutAdjointBatch(none, x, g, b, a, 0, nullptr, 0);
    status_ok("adjoint status");
    fetch(mode ? "gq0_tool" : "gq0", d_vec[0], cnt);
    fetch(mode ? "gdq0_tool" : "gdq0", d_vec[1], cnt);
    fetch(mode ? "gtau_tool" : "gtau", d_gtau, (size_t)T * cnt);
    fetch(mode ? "gext_tool" : "gext", mode ? d_etool : d_eall, mode ? htool.size() : hall.size());
    (void)hipFree(d_gtau);
  }
  // a wrench gradient without wrenches throws what the batch methods throw for invalid arguments
  bool threw = false;
  try
  {
    const rdyn_ext_wrenches no_w = {nullptr, -1, 0};
    chain->getJointAccelerationVjpBatch(none, no_w, b, d_tau, d_seed, d_vec[0], nullptr, nullptr, d_eall, nullptr, d_st, 0, nullptr, 0);
  }
  catch (const std::invalid_argument&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception on ext_bar without wrenches");
  for (double* p : d_vec) (void)hipFree(p);
  for (double* p : {d_q, d_dq, d_tau, d_seed, d_all, d_tool, d_eall, d_etool, d_qt, d_dqt}) (void)hipFree(p);
  (void)hipFree(d_st);
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
