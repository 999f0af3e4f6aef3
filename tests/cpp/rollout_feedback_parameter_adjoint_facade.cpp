// The parameter gradients of a closed-loop rollout through the C++ facade (rosdyn_chain_facade.hpp): rolloutBatch and the
// rolloutParameterAdjointBatch / rolloutParameterAdjointWorkspaceBytes overloads that take a rdyn_feedback (shared gains, limits, a
// reference per step, the digital controller), on inputs that are exact binary fractions; prints every result with 17 digits for
// tests/test_rollout_feedback_parameter_adjoint_facade.py to compare with the Python binding's.  Mode 0 asks for the law's gradients,
// mode 1 passes a null rdyn_feedback_gradient: no law gradient is written and no seed on the command record is read.
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

static double* device_copy(const std::vector<double>& h)
{
  double* d = nullptr;
  HIP_OK(hipMalloc((void**)&d, h.size() * sizeof(double)));
  HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  return d;
}

static double* device_zeros(size_t count)
{
  double* d = nullptr;
  HIP_OK(hipMalloc((void**)&d, count * sizeof(double)));
  HIP_OK(hipMemset(d, 0, count * sizeof(double)));
  return d;
}

static void run(const char* urdf, const char* base, const char* tool)
{
  rosdyn::ChainPtr chain = rosdyn::createChain(slurp(urdf), base, tool, {0.0, 0.0, -9.806});
  const int n = (int)chain->getActiveJointsNumber();
  const int N = 5, T = 3;
  const size_t cnt = (size_t)N * n;
  std::vector<double> hq(cnt), hdq(cnt), htau(cnt * T), hseed(cnt), hqr(cnt * T), hdqr(cnt * T), hgu(cnt * T), hkp(n), hkd(n), hlim(n);
  for (int s = 0; s < N; ++s)
  {
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      hseed[(size_t)s * n + i] = value(s, i, 9);
      for (int t = 0; t < T; ++t)
      {
        htau[t * cnt + (size_t)s * n + i] = 0.5 * value(s, i, 2 + t);
        hqr[t * cnt + (size_t)s * n + i] = value(s, i, 0) + 0.25 * value(s, i, 20 + t);
        hdqr[t * cnt + (size_t)s * n + i] = value(s, i, 1) + 0.25 * value(s, i, 24 + t);
        hgu[t * cnt + (size_t)s * n + i] = value(s, i, 28 + t);
      }
    }
  }
  for (int i = 0; i < n; ++i)
  {
    hkp[i] = 2.0 + 0.25 * i;
    hkd[i] = 0.5 + 0.125 * i;
    hlim[i] = 0.75;
  }
  double *d_q = device_copy(hq), *d_dq = device_copy(hdq), *d_tau = device_copy(htau), *d_seed = device_copy(hseed), *d_qr = device_copy(hqr),
         *d_dqr = device_copy(hdqr), *d_gu = device_copy(hgu), *d_kp = device_copy(hkp), *d_kd = device_copy(hkd), *d_lim = device_copy(hlim);
  // n-vectors per sample: gq0 | gdq0 | gkp | gkd | glim | the end state of the forward call (2); sequences: q_traj | dq_traj | gtau | gq_ref | gdq_ref
  std::vector<double*> d_vec(7), d_seq(5);
  for (double*& p : d_vec) p = device_zeros(cnt);
  for (double*& p : d_seq) p = device_zeros((size_t)T * cnt);
  const size_t P = 10 * (size_t)chain->getJointsNumber();
  double* d_gpi = device_zeros(P);
  int32_t* d_st = nullptr;
  HIP_OK(hipMalloc((void**)&d_st, N * sizeof(int32_t)));
  rdyn_batch b;
  std::memset(&b, 0, sizeof b);
  b.n_samples = N;
  b.q = d_q;
  b.dq = d_dq;
  b.layout = RDYN_LAYOUT_SAMPLE_MAJOR;
  b.device = -1;
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
  rdyn_feedback fb;
  std::memset(&fb, 0, sizeof fb);
  fb.q_ref = d_qr;
  fb.dq_ref = d_dqr;
  fb.ref_step_stride = (int64_t)cnt;
  fb.kp = d_kp;
  fb.kd = d_kd;
  fb.hold = 1;
  fb.tau_limit = d_lim;
  for (int mode = 0; mode < 2; ++mode)
  {
    const rdyn_ext_wrenches* x = nullptr;
    rdyn_rollout_desc f;
    std::memset(&f, 0, sizeof f);
    f.n_steps = T;
    f.integrator = RDYN_INTEGRATOR_RK4;
    f.dt = 1e-3;
    f.tau = d_tau;
    f.tau_step_stride = (int64_t)cnt;
    f.q_end = d_vec[5];
    f.dq_end = d_vec[6];
    f.status = d_st;
    f.q_traj = d_seq[0];
    f.dq_traj = d_seq[1];
    f.traj_step_stride = (int64_t)cnt;
    f.traj_every = 1;
    if (chain->rolloutWorkspaceBytes(f, x, fb, N, 0) != 0) throw std::runtime_error("a swept chain needs no workspace");
    chain->rolloutBatch(none, x, fb, b, f, 0, nullptr, 0);
    status_ok("rollout status");
    rdyn_rollout_adjoint_desc a;
    std::memset(&a, 0, sizeof a);
    a.n_steps = T;
    a.integrator = RDYN_INTEGRATOR_RK4;
    a.dt = 1e-3;
    a.tau = d_tau;
    a.tau_step_stride = (int64_t)cnt;
    a.q_traj = d_seq[0];
    a.dq_traj = d_seq[1];
    a.traj_step_stride = (int64_t)cnt;
    a.gq_end = d_seed;
    a.gq0 = d_vec[0];
    a.gdq0 = d_vec[1];
    a.gtau = d_seq[2];
    a.gtau_step_stride = (int64_t)cnt;
    a.status = d_st;
    rdyn_feedback_gradient g;
    std::memset(&g, 0, sizeof g);
    g.gq_ref = d_seq[3];
    g.gdq_ref = d_seq[4];
    g.gref_step_stride = (int64_t)cnt;
    g.gkp = d_vec[2];
    g.gkd = d_vec[3];
    g.glim = d_vec[4];
    g.gu_traj = d_gu;
    g.gu_step_stride = (int64_t)cnt;
    const rdyn_parameter_gradient pg = {d_gpi, nullptr, 0};
    const size_t bytes = chain->rolloutParameterAdjointWorkspaceBytes(none, a, fb, N, 0);
    if (bytes == 0 || bytes != chain->rolloutParameterAdjointWorkspaceBytes(none, a, N, 0))
      throw std::runtime_error("the workspace is the open-loop call's accumulators");
    void* ws = nullptr;
    HIP_OK(hipMalloc(&ws, bytes));
    chain->rolloutParameterAdjointBatch(none, fb, mode ? nullptr : &g, b, a, pg, 0, ws, bytes);
    status_ok("adjoint status");
    HIP_OK(hipFree(ws));
    const std::string sfx = mode ? "_bare" : "";
    fetch(("gpi" + sfx).c_str(), d_gpi, P);
    fetch(("gq0" + sfx).c_str(), d_vec[0], cnt);
    fetch(("gdq0" + sfx).c_str(), d_vec[1], cnt);
    fetch(("gtau" + sfx).c_str(), d_seq[2], (size_t)T * cnt);
    fetch(("gq_ref" + sfx).c_str(), d_seq[3], (size_t)T * cnt);
    fetch(("gdq_ref" + sfx).c_str(), d_seq[4], (size_t)T * cnt);
    fetch(("gkp" + sfx).c_str(), d_vec[2], cnt);
    fetch(("gkd" + sfx).c_str(), d_vec[3], cnt);
    fetch(("glim" + sfx).c_str(), d_vec[4], cnt);
  }
  // a limit gradient without limits throws what the batch methods throw for invalid arguments
  bool threw = false;
  try
  {
    rdyn_feedback no_lim = fb;
    no_lim.tau_limit = nullptr;
    rdyn_rollout_adjoint_desc a;
    std::memset(&a, 0, sizeof a);
    a.n_steps = 1;
    a.integrator = RDYN_INTEGRATOR_RK4;
    a.dt = 1e-3;
    a.tau = d_tau;
    a.gq0 = d_vec[0];
    rdyn_feedback_gradient g;
    std::memset(&g, 0, sizeof g);
    g.glim = d_vec[4];
    const rdyn_parameter_gradient pg = {d_gpi, nullptr, 0};
    chain->rolloutParameterAdjointBatch(none, no_lim, &g, b, a, pg, 0, nullptr, 0);
  }
  catch (const std::invalid_argument&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception on glim without limits");
  for (double* p : d_vec) (void)hipFree(p);
  for (double* p : d_seq) (void)hipFree(p);
  for (double* p : {d_q, d_dq, d_tau, d_seed, d_qr, d_dqr, d_gu, d_kp, d_kd, d_lim, d_gpi}) (void)hipFree(p);
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
