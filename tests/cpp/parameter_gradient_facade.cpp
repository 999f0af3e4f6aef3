// The parameter gradients through the C++ facade (rosdyn_chain_facade.hpp): withParameters, getJointAccelerationParameterVjpBatch and
// rolloutParameterAdjointBatch with their workspace queries, on inputs that are exact binary fractions; prints every result with 17 digits
// for tests/test_parameter_gradient_facade.py to compare with the Python binding's.  Compiles against the stand-in Eigen headers
// (tests/mock_include) like its siblings.
// usage: prog chain.urdf base tool
#include <cstdio>
#include <fstream>
#include <limits>
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

static void print(const char* what, const double* dev, size_t count)
{
  std::vector<double> v(count);
  HIP_OK(hipMemcpy(v.data(), dev, count * sizeof(double), hipMemcpyDeviceToHost));
  std::printf("%s", what);
  for (double x : v) std::printf(" %.17g", x);
  std::printf("\n");
}

static double* device(const std::vector<double>& h)
{
  double* d = nullptr;
  HIP_OK(hipMalloc((void**)&d, h.size() * sizeof(double)));
  HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  return d;
}

static void run(const char* urdf, const char* base, const char* tool)
{
  rosdyn::ChainPtr nominal = rosdyn::createChain(slurp(urdf), base, tool, {0.0, 0.0, -9.806});
  const int n = (int)nominal->getActiveJointsNumber();
  const int P = 10 * (int)nominal->getJointsNumber();
  // the model: every parameter moved by an exact binary fraction of itself
  rosdyn::VectorXd pi0 = nominal->getNominalParameters();
  std::vector<double> pi(P);
  for (int k = 0; k < P; ++k) pi[k] = pi0(k) * (1.0 + ((k * 5) % 9 - 4) / 64.0);
  rosdyn::ChainPtr chain = nominal->withParameters(pi);
  rosdyn::VectorXd back = chain->getNominalParameters(), still = nominal->getNominalParameters();
  for (int k = 0; k < P; ++k)
    if (back(k) != pi[k] || still(k) != pi0(k)) throw std::runtime_error("withParameters: the parameters do not come back, or the original moved");
  if (chain->getActiveJointsNumber() != nominal->getActiveJointsNumber()) throw std::runtime_error("withParameters: another joint selection");
  const int N = 5, T = 3;
  std::vector<rdyn_component> comps(2);
  std::memset(comps.data(), 0, comps.size() * sizeof(rdyn_component));
  comps[0].type = RDYN_COMP_FRICTION1; comps[0].joint = 0; comps[0].min_velocity = 0.0625; comps[0].max_velocity = 0.75;
  comps[0].parameters[0] = 0.25; comps[0].parameters[1] = 0.5;
  comps[1].type = RDYN_COMP_SPRING; comps[1].joint = n - 1; comps[1].parameters[0] = 1.5; comps[1].parameters[1] = -0.25;
  const int K = rdyn_components_columns(comps.data(), (int)comps.size());
  const size_t cnt = (size_t)N * n;
  std::vector<double> hq(cnt), hdq(cnt), htau(cnt * T), hgq(cnt), hgv(cnt);
  for (int s = 0; s < N; ++s)
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      hgq[(size_t)s * n + i] = value(s, i, 9);
      hgv[(size_t)s * n + i] = value(s, i, 10);
      for (int t = 0; t < T; ++t) htau[t * cnt + (size_t)s * n + i] = 0.5 * value(s, i, 2 + t);
    }
  double *d_q = device(hq), *d_dq = device(hdq), *d_tau = device(htau), *d_gq = device(hgq), *d_gv = device(hgv);
  std::vector<double> zeros(cnt * T, 0.0), zp((size_t)N * (P + K), 0.0);
  double *d_qb = device(hq), *d_vb = device(hq), *d_tb = device(hq), *d_ddq = device(hq);
  double *d_qt = device(zeros), *d_vt = device(zeros), *d_gtau = device(zeros), *d_qe = device(hq), *d_ve = device(hq);
  double *d_rows = device(zp), *d_crows = device(zp), *d_gpi = device(zp), *d_gcomp = device(zp);
  int32_t* d_st = nullptr;
  HIP_OK(hipMalloc((void**)&d_st, N * sizeof(int32_t)));
  rdyn_batch b;
  std::memset(&b, 0, sizeof b);
  b.n_samples = N;
  b.q = d_q;
  b.dq = d_dq;
  b.layout = RDYN_LAYOUT_SAMPLE_MAJOR;
  b.device = -1;
  rdyn_rollout_desc f;
  std::memset(&f, 0, sizeof f);
  f.n_steps = T;
  f.integrator = RDYN_INTEGRATOR_RK4;
  f.dt = 1e-3;
  f.tau = d_tau;
  f.tau_step_stride = (int64_t)cnt;
  f.q_end = d_qe;
  f.dq_end = d_ve;
  f.q_traj = d_qt;
  f.dq_traj = d_vt;
  f.traj_step_stride = (int64_t)cnt;
  f.traj_every = 1;
  f.status = d_st;
  rdyn_rollout_adjoint_desc a;
  std::memset(&a, 0, sizeof a);
  a.n_steps = T;
  a.integrator = RDYN_INTEGRATOR_RK4;
  a.dt = 1e-3;
  a.tau = d_tau;
  a.tau_step_stride = (int64_t)cnt;
  a.q_traj = d_qt;
  a.dq_traj = d_vt;
  a.traj_step_stride = (int64_t)cnt;
  a.gq_end = d_gq;
  a.gdq_end = d_gv;
  a.gq0 = d_qb;
  a.gdq0 = d_vb;
  a.gtau = d_gtau;
  a.gtau_step_stride = (int64_t)cnt;
  a.status = d_st;
  size_t ws_bytes = chain->rolloutParameterAdjointWorkspaceBytes(comps, a, N, 0);
  const size_t fwd_bytes = chain->rolloutWorkspaceBytes(f, N, 0), one_bytes = chain->getJointAccelerationParameterVjpWorkspaceBytes(comps, N, 0);
  if (ws_bytes == 0 || one_bytes == 0) throw std::runtime_error("the parameter gradients need a workspace");
  if (fwd_bytes > ws_bytes) ws_bytes = fwd_bytes;
  if (one_bytes > ws_bytes) ws_bytes = one_bytes;
  void* ws = nullptr;
  HIP_OK(hipMalloc(&ws, ws_bytes));
  std::vector<int32_t> hst(N);
  auto status_ok = [&](const char* what) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(hst.data(), d_st, N * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int s = 0; s < N; ++s)
      if (hst[s] != 1) throw std::runtime_error(what);
  };
  chain->rolloutBatch(comps, b, f, 0, ws, ws_bytes);
  status_ok("rollout status");
  rdyn_parameter_gradient pg;
  pg.gpi = d_gpi;
  pg.gcomp = d_gcomp;
  pg.accumulate = 0;
  chain->rolloutParameterAdjointBatch(comps, b, a, pg, 0, ws, ws_bytes);
  status_ok("adjoint status");
  print("gq0", d_qb, cnt);
  print("gdq0", d_vb, cnt);
  print("gtau", d_gtau, cnt * T);
  print("gpi", d_gpi, P);
  print("gcomp", d_gcomp, K);
  chain->getJointAccelerationParameterVjpBatch(comps, b, d_tau, d_gq, d_rows, d_crows, d_gpi, d_gcomp, false, d_tb, d_ddq, d_st, 0, ws, ws_bytes);
  status_ok("product status");
  print("pi_bar", d_rows, (size_t)N * P);
  print("comp_bar", d_crows, (size_t)N * K);
  print("pi_bar_sum", d_gpi, P);
  print("comp_bar_sum", d_gcomp, K);
  print("tau_bar", d_tb, cnt);
  print("ddq", d_ddq, cnt);
  // invalid arguments throw what the other batch methods throw for them
  int threw = 0;
  try
  {
    chain->getJointAccelerationParameterVjpBatch(comps, b, d_tau, d_gq, nullptr, nullptr, nullptr, nullptr, false, nullptr, d_ddq, d_st, 0, ws, ws_bytes);
  }
  catch (const std::invalid_argument&)
  {
    ++threw;
  }
  pg.gpi = pg.gcomp = nullptr;
  try
  {
    chain->rolloutParameterAdjointBatch(comps, b, a, pg, 0, ws, ws_bytes);
  }
  catch (const std::invalid_argument&)
  {
    ++threw;
  }
  pi[3] = std::numeric_limits<double>::quiet_NaN();
  try
  {
    nominal->withParameters(pi);
  }
  catch (const std::invalid_argument&)
  {
    ++threw;
  }
  if (threw != 3) throw std::runtime_error("no exception on every product null / no gradient selected / a parameter that is not finite");
  for (double* p : {d_q, d_dq, d_tau, d_gq, d_gv, d_qb, d_vb, d_tb, d_ddq, d_qt, d_vt, d_gtau, d_qe, d_ve, d_rows, d_crows, d_gpi, d_gcomp}) (void)hipFree(p);
  (void)hipFree(d_st);
  (void)hipFree(ws);
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
