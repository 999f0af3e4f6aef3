// Derivatives of the joint torque through the C++ facade (rosdyn_chain_facade.hpp): the batch method getJointTorqueDerivativesBatch and the
// single-sample getter getJointTorqueDerivatives, on a chain swept in registers (ur10_like, 6 joints), on one with input joints out of
// chain order (ur10_public, 4 of 6) and on one with 14 input joints (the rolled kernel).
// usage: prog ur10_like.urdf ur10_public.urdf rev14.urdf
// Checks: single sample == batch; the batch's M == getJointInertia; every column against a central difference of the facade's own
// getJointTorque with step h = 1e-5: truncation h^2 / 6 |tau'''| ~ 1.3e-10 A (tau is a trigonometric polynomial of degree 2 in q_k with
// amplitude A: |tau'''| <= 8 A; exact in Dq_k, a quadratic), rounding eps |tau| / h ~ 2e-11 |tau| -- bound 1e-7 (max|D| + |tau|_inf): a wrong
// term shows at order 1, and the amplitude of a harmonic may exceed the sample's own |tau| and |D| by a few hundred.
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

static void check_chain(rosdyn::ChainPtr chain)
{
  const int n = (int)chain->getActiveJointsNumber();
  const int N = 300;
  const size_t nn = (size_t)n * n;
  std::vector<double> hq((size_t)N * n), hdq(hq.size()), hddq(hq.size());
  for (int s = 0; s < N; ++s)
    for (int i = 0; i < n; ++i)
    {
      hq[(size_t)s * n + i] = value(s, i, 0);
      hdq[(size_t)s * n + i] = value(s, i, 1);
      hddq[(size_t)s * n + i] = 3.0 * value(s, i, 2);
    }
  // ---- the batch method
  double *d_q = nullptr, *d_dq = nullptr, *d_ddq = nullptr, *d_out = nullptr;
  const size_t bytes = hq.size() * sizeof(double), obytes = (size_t)N * nn * sizeof(double);
  HIP_OK(hipMalloc((void**)&d_q, bytes));
  HIP_OK(hipMalloc((void**)&d_dq, bytes));
  HIP_OK(hipMalloc((void**)&d_ddq, bytes));
  HIP_OK(hipMalloc((void**)&d_out, 3 * obytes));
  HIP_OK(hipMemcpy(d_q, hq.data(), bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_dq, hdq.data(), bytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_ddq, hddq.data(), bytes, hipMemcpyHostToDevice));
  rdyn_batch b;
  std::memset(&b, 0, sizeof b);
  b.n_samples = N;
  b.q = d_q;
  b.dq = d_dq;
  b.ddq = d_ddq;
  b.layout = RDYN_LAYOUT_SAMPLE_MAJOR;
  b.device = -1;
  chain->getJointTorqueDerivativesBatch(b, d_out, d_out + (size_t)N * nn, d_out + 2 * (size_t)N * nn);
  HIP_OK(hipDeviceSynchronize());
  std::vector<double> hout(3 * (size_t)N * nn);
  HIP_OK(hipMemcpy(hout.data(), d_out, 3 * obytes, hipMemcpyDeviceToHost));
  const double* const bq = hout.data();
  const double* const bv = hout.data() + (size_t)N * nn;
  const double* const bm = hout.data() + 2 * (size_t)N * nn;
  // ---- the single-sample getter on three of the samples
  const int picks[3] = {0, 137, N - 1};
  const double h = 1e-5;
  for (int p = 0; p < 3; ++p)
  {
    const int s = picks[p];
    rosdyn::VectorXd q(n), dq(n), ddq(n);
    for (int i = 0; i < n; ++i)
    {
      q(i) = hq[(size_t)s * n + i];
      dq(i) = hdq[(size_t)s * n + i];
      ddq(i) = hddq[(size_t)s * n + i];
    }
    rosdyn::MatrixXd Dq_, Dv_;
    chain->getJointTorqueDerivatives(q, dq, ddq, Dq_, Dv_);
    if (Dq_.rows() != n || Dq_.cols() != n || Dv_.rows() != n || Dv_.cols() != n) throw std::runtime_error("single: size");
    const rosdyn::MatrixXd M = chain->getJointInertia(q);
    const rosdyn::VectorXd tau0 = chain->getJointTorque(q, dq, ddq);
    double scale = 0.0;
    for (int i = 0; i < n; ++i) scale = std::fmax(scale, std::fabs(tau0(i)));
    double dmax = 0.0;
    for (int k = 0; k < n; ++k)
      for (int i = 0; i < n; ++i) dmax = std::fmax(dmax, std::fmax(std::fabs(Dq_(i, k)), std::fabs(Dv_(i, k))));
    scale += dmax;
    for (int k = 0; k < n; ++k)
    {
      for (int i = 0; i < n; ++i)
      {
        const size_t e = (size_t)s * nn + (size_t)i + (size_t)n * k;
        if (std::fabs(Dq_(i, k) - bq[e]) > 1e-12 * scale || std::fabs(Dv_(i, k) - bv[e]) > 1e-12 * scale) throw std::runtime_error("single != batch");
        if (std::fabs(M(i, k) - bm[e]) > 1e-11 * std::fmax(1.0, std::fabs(M(i, k)))) throw std::runtime_error("batch M != getJointInertia");
      }
      for (int which = 0; which < 2; ++which)
      {
        rosdyn::VectorXd xp = which == 0 ? q : dq, xm = xp;
        xp(k) += h;
        xm(k) -= h;
        const rosdyn::VectorXd tp = which == 0 ? chain->getJointTorque(xp, dq, ddq) : chain->getJointTorque(q, xp, ddq);
        const rosdyn::VectorXd tm = which == 0 ? chain->getJointTorque(xm, dq, ddq) : chain->getJointTorque(q, xm, ddq);
        for (int i = 0; i < n; ++i)
        {
          const double fd = (tp(i) - tm(i)) / (2.0 * h);
          const double got = which == 0 ? Dq_(i, k) : Dv_(i, k);
          if (!(std::fabs(fd - got) <= 1e-7 * scale))
          {
            std::fprintf(stderr, "sample %d %s(%d, %d): %.12g against the central difference %.12g (scale %.3g)\n", s, which ? "dtau_dDq" : "dtau_dq", i, k,
                         got, fd, scale);
            throw std::runtime_error("derivative against the central difference");
          }
        }
      }
    }
  }
  // every output null is refused
  bool threw = false;
  try
  {
    chain->getJointTorqueDerivativesBatch(b, nullptr, nullptr, nullptr);
  }
  catch (const std::exception&)
  {
    threw = true;
  }
  if (!threw) throw std::runtime_error("no exception when every output is null");
  (void)hipFree(d_q);
  (void)hipFree(d_dq);
  (void)hipFree(d_ddq);
  (void)hipFree(d_out);
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
    check_chain(rosdyn::createChain(slurp(argv[1]), "base_link", "tool0", {0.0, 0.0, -9.806}));
    rosdyn::ChainPtr perm = rosdyn::createChain(slurp(argv[2]), "base_link", "tool0", {0.0, 0.0, -9.806});
    if (!perm->setInputJointsName({"wrist_1_joint", "shoulder_pan_joint", "elbow_joint", "shoulder_lift_joint"})) throw std::runtime_error("setInputJointsName");
    check_chain(perm);
    check_chain(rosdyn::createChain(slurp(argv[3]), "l0", "l14", {0.0, 0.0, -9.806}));
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
