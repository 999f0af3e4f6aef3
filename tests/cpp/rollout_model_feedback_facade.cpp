// Closed-loop rollouts under a model-based law through the C++ facade (rosdyn_chain_facade.hpp): rolloutWorkspaceBytes / rolloutBatch with
// a rdyn_feedback and a rdyn_model_feedback whose model is withParameters of a perturbed parameter vector -- computed torque with limits
// and a command record, then gravity compensation with the tool's wrench -- on inputs that are exact binary fractions; prints every result
// with 17 digits for tests/test_rollout_model_feedback_facade.py to compare with the Python binding's.
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
  const int n = (int)chain->getActiveJointsNumber();
  // the controller's model: every parameter off by up to 6.25 %
  std::vector<double> pi(10 * (size_t)chain->getJointsNumber());
  if (rdyn_nominal_parameters(chain->handle(), pi.data()) != RDYN_OK) throw std::runtime_error("nominal parameters");
  for (size_t i = 0; i < pi.size(); ++i) pi[i] *= 1.0 + ((double)((i * 5) % 9) - 4.0) / 64.0;
  rosdyn::ChainPtr model = chain->withParameters(pi);
  const int N = 5, T = 3;
  const size_t cnt = (size_t)N * n, bytes = cnt * sizeof(double);
  std::vector<double> hq(cnt), hdq(cnt), htau(cnt * T), hqr(cnt * T), hdqr(cnt * T), hddqr(cnt * T), htool((size_t)N * 6), hkp(n), hkd(n), hlim(n), out(cnt);
  for (int s = 0; s < N; ++s)
  {
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      for (int t = 0; t < T; ++t)
      {
        htau[t * cnt + (size_t)s * n + i] = 0.5 * value(s, i, 2 + t);
        hqr[t * cnt + (size_t)s * n + i] = value(s, i, 20 + t);
        hdqr[t * cnt + (size_t)s * n + i] = value(s, i, 30 + t);
        hddqr[t * cnt + (size_t)s * n + i] = value(s, i, 40 + t);
      }
    }
    for (int e = 0; e < 6; ++e) htool[(size_t)s * 6 + e] = 0.5 * value(s, e, 12);
  }
  for (int i = 0; i < n; ++i)
  {
    hkp[i] = 4.0 + i;
    hkd[i] = 0.5 + 0.25 * i;
    hlim[i] = 2.0;
  }
  double *d_q = device_copy(hq), *d_dq = device_copy(hdq), *d_tau = device_copy(htau), *d_qr = device_copy(hqr), *d_dqr = device_copy(hdqr), *d_ddqr = device_copy(hddqr);
  double *d_tool = device_copy(htool), *d_kp = device_copy(hkp), *d_kd = device_copy(hkd), *d_lim = device_copy(hlim);
  double *d_qe = nullptr, *d_dqe = nullptr, *d_ut = nullptr;
  int32_t* d_st = nullptr;
  void* ws = nullptr;
  HIP_OK(hipMalloc((void**)&d_qe, bytes));
  HIP_OK(hipMalloc((void**)&d_dqe, bytes));
  HIP_OK(hipMalloc((void**)&d_ut, bytes * T));
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
  d.traj_every = 1;
  d.traj_step_stride = (int64_t)cnt;
  d.status = d_st;
  rdyn_feedback fb;
  std::memset(&fb, 0, sizeof fb);
  fb.q_ref = d_qr;
  fb.dq_ref = d_dqr;
  fb.ref_step_stride = (int64_t)cnt;
  fb.kp = d_kp;
  fb.kd = d_kd;
  fb.hold = 1;
  fb.tau_limit = d_lim;
  fb.tau_traj = d_ut;
  rdyn_model_feedback mfb;
  std::memset(&mfb, 0, sizeof mfb);
  mfb.model = model->handle();
  mfb.law = RDYN_LAW_COMPUTED_TORQUE;
  mfb.ddq_ref = d_ddqr;
  const rdyn_ext_wrenches tool_w = {d_tool, (int32_t)chain->getJointsNumber(), 0};
  const std::vector<rdyn_component> none;
  const size_t ws_bytes = chain->rolloutWorkspaceBytes(d, &tool_w, fb, mfb, N, 0);
  if (ws_bytes != 0 || chain->rolloutWorkspaceBytes(d, nullptr, fb, mfb, N, 0) != 0) throw std::runtime_error("workspace queries");
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
  chain->rolloutBatch(none, nullptr, fb, mfb, b, d, 0, ws, ws_bytes);
  status_ok("closed-loop status");
  fetch("q_end", d_qe);
  fetch("dq_end", d_dqe);
  fetch("u_last", d_ut + (size_t)(T - 1) * cnt);
  fb.hold = 0;
  mfb.law = RDYN_LAW_GRAVITY_COMPENSATION;
  mfb.ddq_ref = nullptr;
  chain->rolloutBatch(none, &tool_w, fb, mfb, b, d, 0, ws, ws_bytes);
  status_ok("closed-loop status, tool wrench");
  fetch("q_end_tool", d_qe);
  fetch("dq_end_tool", d_dqe);
  // an argument error throws what the batch methods throw for invalid arguments
  bool threw = false;
  try
  {
    mfb.ddq_ref = d_ddqr;  // gravity compensation takes no acceleration reference
    chain->rolloutBatch(none, nullptr, fb, mfb, b, d, 0, ws, ws_bytes);
  }
  catch (const std::invalid_argument&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception on ddq_ref with gravity compensation");
  for (double* p : {d_q, d_dq, d_tau, d_qr, d_dqr, d_ddqr, d_tool, d_kp, d_kd, d_lim, d_qe, d_dqe, d_ut}) (void)hipFree(p);
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
