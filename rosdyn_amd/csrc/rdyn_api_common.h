// rdyn_api_common.h -- what the translation units of the C-ABI layer (rdyn_api.cpp, rdyn_api_dynamics.cpp, rdyn_api_gram.cpp,
// rdyn_api_tsqr.cpp) share: error / device plumbing, chain-constant residency, the batch checks, strides, and the tile and chunk helpers
// of the Gram and factor calls.  Every item is declared here once and defined inline or in the one file named beside it; nothing here
// is exported.
//
// Diagnostic environment switches exist ONLY in builds compiled with -DRDYN_ENABLE_PROBES (tools/build_variant.sh).  The shipped
// library never reads the environment: a variable left over from a profiling shell cannot change results
// (tests/test_release_object.py).  A switch lives here only while a tool outside tools/archive/ sets it; this is the whole list:
//   RDYN_GRAM_PATH=image    rdyn_regressor_gram: the global-image kernel (rdyn_fused_gram.hip) where the wave-pair kernel would
//                           run (tools/probe_gram_paths.py; the third route, two kernels, is the chunk_samples argument)
#ifndef RDYN_API_COMMON_H
#define RDYN_API_COMMON_H

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include <hip/hip_runtime.h>

#include "rdyn_chain.hpp"
#include "rdyn_kernels.h"

#pragma GCC visibility push(hidden)

#ifdef RDYN_ENABLE_PROBES
inline const char* probe_env(const char* name) { return getenv(name); }
#else
inline const char* probe_env(const char*) { return nullptr; }
#endif

#define RDYN_HIP_TRY(expr)                                                     \
  do                                                                           \
  {                                                                            \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
    {                                                                          \
      rdyn_set_error("HIP error: %s (%s)", hipGetErrorString(_e), #expr);      \
      return RDYN_ERR_HIP;                                                     \
    }                                                                          \
  } while (0)

struct DeviceGuard
{
  int prev = -1;
  bool switched = false;
  int enter(int device)
  {
    if (hipGetDevice(&prev) != hipSuccess)
    {
      rdyn_set_error("no HIP device available (hipGetDevice failed)");
      return RDYN_ERR_NO_DEVICE;
    }
    if (device >= 0 && device != prev)
    {
      if (hipSetDevice(device) != hipSuccess)
      {
        rdyn_set_error("hipSetDevice(%d) failed", device);
        return RDYN_ERR_NO_DEVICE;
      }
      switched = true;
    }
    return RDYN_OK;
  }
  ~DeviceGuard()
  {
    if (switched) (void)hipSetDevice(prev);
  }
};

// ---- rdyn_api.cpp ----------------------------------------------------------------------------------------------
// the device copy of a chain's constants on the current device, uploaded at first use (device_const: chains the unrolled kernels sweep;
// device_const_long: the run-time-length kernels; device_expand: the expansion blocks X_f of a chain with a reduced companion)
int device_const(const rdyn_chain* c, const RdynChainConst** out);
int device_const_long(const rdyn_chain* c, const RdynLongChainConst** out);
int device_expand(const rdyn_chain* c, const double** out);

// How an entry point serves a chain of more than RDYN_MAX_SWEPT_JOINTS joints: through its reduced companion (regressor, torque,
// inertia, normal equations, R factors, IK: at most RDYN_MAX_SWEPT_JOINTS input joints) or by the run-time-length kinematic kernels
// (frames, Jacobians, twists, wrenches: any number of input joints)
enum { LONG_NONE = 0, LONG_COMPANION = 1, LONG_KERNELS = 2 };
int check_batch(const rdyn_chain* c, const rdyn_batch* b, bool need_dq, bool need_ddq, const char* fn, int long_mode);

// validates the components and copies them with the constructor rules of the reference applied
int fill_components(const rdyn_component* comps, int n_comps, int n_active, RdynComponentArgs* a);

// every non-null pointer starts on a 128-byte line (the staged copy-out of the sample-major records writes whole lines)
template <class... P>
inline bool lines_aligned(P... p)
{
  return (((uintptr_t)p | ...) & 127u) == 0;
}

// per-sample / per-element strides of a record of `elems` doubles
inline void rec_strides(const rdyn_batch* b, int64_t elems, int64_t* ss, int64_t* se)
{
  if (b->layout == RDYN_LAYOUT_SAMPLE_MAJOR)
  {
    *ss = elems;
    *se = 1;
  }
  else
  {
    *ss = 1;
    *se = b->n_samples;
  }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// temporary normal equations of the reduced chain at the end of a Gram workspace: G_red | c_red | bb_red
inline size_t reduce_tmp_bytes(int cols_red) { return align256(((size_t)cols_red * cols_red + cols_red + 1) * sizeof(double)); }

// ---- rdyn_api_dynamics.cpp -------------------------------------------------------------------------------------
// RDYN_OK, or the refusal of the rolled derivative kernel (k_long_torque_deriv) on a device that grants a workgroup too little LDS.
// The per-joint state of a workgroup's samples must fit the LDS the batch's device grants one workgroup (the runtime's figure, read once
// per device): a launch that asks for more fails without a trace.  gfx950 grants 160 KB and RDYN_MAX_JOINTS joints ask for 108 KB, so
// this answer is for devices with less (64 KB: chains beyond 18 joints).  The batch's device must be current.
int long_deriv_lds_refusal(const rdyn_chain* c, const char* who);

// ---- rdyn_api_gram.cpp: what the Gram and the factor calls share -------------------------------------------------
inline int64_t default_chunk(int64_t chunk) { return chunk > 0 ? chunk : 32768; }
// samples per chunk image [Y | C | tau_meas] (`cols` columns in front of tau_meas) of the wide normal equations and the wide R factors
int64_t wide_chunk(const rdyn_chain* c, int cols, int64_t chunk_samples);
inline size_t panel_slab_bytes(int n_cols) { return align256(rdyn_panel_gram_slab_bytes(n_cols)); }
// run_flag: null, or a device word that lets both kernels leave at once (the rounds of the panel QR)
int panel_gram_launch(const double* A, int64_t rows, int64_t lda, int n_cols, const double* bvec, double* G, double* cvec, double* bb,
                      int slab_accumulate, bool finish, int add_to_output, void* slabs, const int* run_flag, hipStream_t st,
                      int64_t row_block = 0, const int* first_col = nullptr, int n_row_blocks = 0);
// the expansion of the reduced companion (n_red joints, K component columns riding along) back onto chain c: everything of
// RdynGramExpandArgs but the matrices it reads and writes
int fill_expand_args(const rdyn_chain* c, int n_red, int K, RdynGramExpandArgs* ea);

// The element-major chunk image [Y (10 nJ) | C (K) | tau_meas] of cnt samples s0, s0 + S, s0 + 2 S, ... (S = sample_stride): rows
// j * cnt + s, lda = n * cnt, tau_meas in column `cols` (without tau_meas that column is not written).  Y by k_long_regressor
// (rdyn_long_local.hip) when dl is set -- more input joints than the unrolled kernels sweep --, by the element-major regressor sweep
// otherwise; the component columns behind it.  The sweep does not store the structural zeros (rows of input joint j left of column
// 10 * its chain index), and 16-row groups that straddle two row blocks read a few of them: unless `clear` is off, write() zeroes the
// whole image first wherever its layout changes (first chunk, shorter last chunk).
struct ChunkImage
{
  const rdyn_chain* c;
  const rdyn_batch* b;
  const double* tau_meas;
  double* image;
  int cols;
  const RdynComponentArgs* ca;  // filled by fill_components: n_comps of them, K columns
  int n_comps, K;
  const RdynChainConst* dc = nullptr;
  const RdynLongChainConst* dl = nullptr;
  bool clear = true;
  int64_t cleared_cnt = -1;  // the chunk length the image was last zeroed for

  ChunkImage(const rdyn_chain* c, const rdyn_batch* b, const double* tau_meas, double* image, int cols, const RdynComponentArgs* ca = nullptr,
             int n_comps = 0, int K = 0)
      : c(c), b(b), tau_meas(tau_meas), image(image), cols(cols), ca(ca), n_comps(n_comps), K(K)
  {
  }
  // the chain constants of the writer, looked up once per call
  int bind(bool long_kernel) { return long_kernel ? device_const_long(c, &dl) : device_const(c, &dc); }
  int write(int64_t s0, int64_t cnt, int64_t sample_stride, hipStream_t stream);
};

// the chain the tile kernels sweep: the sorted view when the input joints were listed out of chain order (rdyn_chain.hpp)
inline const rdyn_chain* ordered(const rdyn_chain* c) { return c->sorted ? c->sorted.get() : c; }
// rows of the row waves of the one-lane-per-sample sweepers (rdyn_kin_sweepers.inc): row l (input joints in chain order) is carried
// through n - l links; longest row first, each to the wave with the least work so far.  The Gram kernel has seven row waves with two
// slots (the one that shares the kinematics wave's SIMD, `skip`, stays empty up to 6 joints), pass B of the R factor three with three.
void fill_sw_rows(RdynLdsGramArgs* la, int n, int waves, int slots, int skip);
void fill_in_map(const rdyn_chain* c, RdynLdsGramArgs* la);
// the one-lane-per-sample sweepers of the wave-pair Gram kernel serve this chain (every joint an input joint): the tile padding they
// use (4, or 2 = the compact layout), 0 = no
int kin_sweeper_pad(const rdyn_chain* c, int n_comp_cols);
// Tile layout of the LDS-resident regressor -> Gram and R-factor kernels (rdyn_duo_gram.hip, rdyn_cholqr.hip, rdyn_tsqr.hip): the columns
// of link f keep the rows of the input joints at chain index <= f; K component columns (one 16-row group each) and the measured
// torque follow.  Returns false when the input joints are not in chain order (the packed rows must be a prefix).
bool build_lds_tile(const rdyn_chain* c, int n_comp_cols, RdynLdsGramArgs* la, bool compact = false);

#pragma GCC visibility pop

#endif
