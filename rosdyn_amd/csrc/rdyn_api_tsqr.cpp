// rdyn_api_tsqr.cpp -- the R factors of the C-ABI (include/rdyn.h): rdyn_tsqr, the regressor and identification factors, their reports,
// and the column-panel (wide) factors.  The chunk images and tile layouts are those of the normal equations (rdyn_api_gram.cpp, through
// rdyn_api_common.h).  The entry points take their C linkage from their declarations in include/rdyn.h.
#include <functional>

#include "rdyn_api_common.h"

// ---- tall-skinny QR: the R factor without forming A'A (rdyn_tsqr.hip, rdyn_tsqr_wide.hip, rdyn_cholqr.hip) ---------------------
static const int kTsqrBlocks = 256;    // persistent workgroups (one per CU), four waves = four running factors each
static const int kCholqrBlocks = 256;
// ~0.2 ms of fixed cost (the subsample's Gram matrix, the two small dense kernels, seven launches that leave at once) + 0.78 / 1.2 ms
// per 1e6 samples (6 / 7 joints) against 0.3 - 0.4 ms + 2.8 / 3.8 ms per 1e6 samples for the Householder route: faster at every
// size measured (2 000 samples: 183 vs 288 us; 200 000: 364 vs 969 us).  Small batches keep the Householder folds -- a few hundred
// rows say little about what a preconditioner built on them is worth, and there is nothing to win.
static const int64_t kCholqrMinTiles = 256;        // fused routes: 4 096 samples
static const int64_t kCholqrMinGroups = 2048;      // rdyn_tsqr: 32 768 rows
static const int64_t kTsqrImageChunk = 65536;      // samples per chunk image of the 9 .. 10-joint factor route (0.53 GB at 10 joints; 16 384: 3x the time per sample -- every chunk pays the fixed cost of a factor call)

// offsets (doubles) of the regions every factor call carves out of its workspace.  Region 1: the Householder route's leaves + tree
// levels (rdyn_tsqr.hip or rdyn_tsqr_wide.hip).  Region 2: the preconditioned route's slabs, W, the intermediate factors and the flags.
struct TsqrLayout
{
  size_t householder_doubles = 0;
  size_t slabs = 0, w = 0, v = 0, r1p = 0, g2 = 0, r_swept = 0, r_full = 0, flag = 0, wide = 0, wide_doubles = 0, total_doubles = 0;
};
// n1: width of the factor that is computed (padded width where the kernels pad); nb: 16-column blocks of the preconditioned route's
// column space (0: that route does not serve the shape); n1_full: width of the expanded factor (0: nothing is expanded)
static TsqrLayout tsqr_layout(size_t householder_doubles, int n1, int nb, int n1_full)
{
  TsqrLayout L;
  L.householder_doubles = householder_doubles;
  size_t off = (L.householder_doubles + 31) & ~(size_t)31;
  auto take = [&](size_t doubles) {
    const size_t at = off;
    off = (off + doubles + 31) & ~(size_t)31;
    return at;
  };
  const int nt = nb * (nb + 1) / 2;
  L.slabs = take((size_t)kCholqrBlocks * nt * 256);
  L.w = take((size_t)nt * 256);
  L.r1p = take((size_t)n1 * n1);
  L.g2 = take((size_t)n1 * n1 + 1);
  L.r_swept = take((size_t)n1 * n1);
  L.v = take((size_t)n1 * n1);
  L.r_full = take((size_t)n1_full * n1_full);  // the expanded factor of a call that accumulates (folded into the caller's afterwards)
  L.flag = take(96);  // ints: [0] run round 1, [1] run the stand-by (Householder) call, [2] run round 0, [16 .. 127] the deferred columns;
                      // doubles [64 .. 69]: gamma (preconditioner), rho, gamma (factor kernel) of the two rounds (diagnostics) -- behind
                      // the 112 column flags (until round 5 at [56 .. 61], on top of the flags of columns 96 .. 107)
  L.wide_doubles = (nb > 0 && n1 > rdyn_cholqr_max_cols_lds()) ? (size_t)2 * n1 * n1 : 0;
  L.wide = take(L.wide_doubles);  // the dense kernels' two n1 x n1 squares where they do not fit the LDS (97 .. 112 columns)
  L.total_doubles = off;
  return L;
}

// The preconditioned CholeskyQR rounds on a Gram matrix of a row subsample that already sits in ws + L.g2 ([G (P x P) | c (P) | bb]):
// two rounds of  precond -> pass B (run_pass_b(W, run_flag, slabs)) -> slab reduction -> factor kernel, the second one and the
// stand-by started by the device only (flags).  R_out <- the accepted factor (n1 x n1).  Shared by the fused routes and rdyn_tsqr.
typedef std::function<int(const double* W, const int* run_flag, double* slabs)> PassB;
static int cholqr_rounds(double* ws, const TsqrLayout& L, int n1, int col_shift, int nb, int slab_nb, int has_b, double row_scale, int blocks,
                         double* R_out, hipStream_t stream, const PassB& run_pass_b)
{
  int* const flag = (int*)(ws + L.flag);
  RdynGramArgs ga;
  memset(&ga, 0, sizeof ga);
  ga.P = n1 - 1;
  ga.slabs = ws + L.slabs;
  ga.G = ws + L.g2;
  ga.c = ws + L.g2 + (size_t)(n1 - 1) * (n1 - 1);
  ga.bb = ga.c + (n1 - 1);
  ga.col_shift = col_shift;
  ga.slab_nb = slab_nb;
  const int n_rounds = 2;
  double* const wide_sq = L.wide_doubles ? ws + L.wide : nullptr;  // factors beyond 96 columns: the dense kernels' two squares
  for (int round = 0; round < n_rounds; ++round)
  {
    // round 0: W from the subsample's Gram matrix.  Round 1 (CholeskyQR2 on top): W from round 0's factor; its kernels leave at once
    // unless round 0's factor kernel asked for it (flag[0]).  Round 0 itself runs when its preconditioner is fit for it (flag[2]).
    const int* const run = round == 0 ? flag + 2 : flag;
    if (round == 0)
      RDYN_HIP_TRY(rdyn_launch_cholqr_precond(nullptr, ga.G, ga.c, ga.bb, n1, col_shift, nb, row_scale, ws + L.r1p, ws + L.w, ws + L.v, flag + 16, flag, 0,
                                              nullptr, ws + L.flag + 64, stream, wide_sq));
    else
      RDYN_HIP_TRY(rdyn_launch_cholqr_precond(R_out, nullptr, nullptr, nullptr, n1, col_shift, nb, 1.0, ws + L.r1p, ws + L.w, ws + L.v, flag + 16, flag, 1,
                                              flag, ws + L.flag + 65, stream, wide_sq));
    int st = run_pass_b(ws + L.w, run, ws + L.slabs);
    if (st != RDYN_OK) return st;
    ga.run_flag = run;
    RDYN_HIP_TRY(rdyn_launch_gram_finish(ga, blocks, stream));
    RDYN_HIP_TRY(rdyn_launch_cholqr_factor(ga.G, ga.c, ga.bb, n1, has_b, ws + L.r1p, ws + L.v, flag + 16, R_out, flag, round, run, ws + L.flag + 66 + round,
                                           stream, wide_sq));
  }
  return RDYN_OK;
}

static void read_report(const double* raw, int n1, rdyn_tsqr_report* out)
{
  int flags[128];
  memcpy(flags, raw, sizeof flags);
  out->route = 1;
  const bool round0 = flags[2] != 0, round1 = round0 && flags[0] != 0;
  out->stage = flags[1] ? 2 : (round1 ? 1 : 0);
  for (int k = 0; k < n1 && 16 + k < 128; ++k) out->n_deferred += flags[16 + k] ? 1 : 0;
  if (round0)
  {
    out->gamma[0] = raw[68];
    out->rho[0] = raw[66];
  }
  if (round1)
  {
    out->gamma[1] = raw[69];
    out->rho[1] = raw[67];
  }
}

// ---- rdyn_tsqr: a materialised matrix
struct TsqrRowsPlan
{
  int n1 = 0, nc_reg = 0, nb = 0;  // nc_reg: padded width of the register-resident folds (0: wider than 64 -> LDS-resident folds)
  bool cholqr_ok = false;          // the dense steps of the preconditioned route hold the factor
  TsqrLayout L;
};
static bool tsqr_rows_plan(int n1, TsqrRowsPlan* p)
{
  if (n1 < 1 || n1 > rdyn_tsqr_wide_max_cols()) return false;
  p->n1 = n1;
  p->nc_reg = rdyn_tsqr_padded_cols(n1);
  p->cholqr_ok = n1 >= 2 && n1 <= rdyn_cholqr_max_cols();
  p->nb = p->cholqr_ok ? (n1 + 15) / 16 : 0;
  size_t hh = rdyn_tsqr_wide_workspace_doubles(n1, kTsqrBlocks);
  if (p->nc_reg)
  {
    const size_t reg = rdyn_tsqr_workspace_doubles(p->nc_reg, kTsqrBlocks);
    if (reg > hh) hh = reg;
  }
  p->L = tsqr_layout(hh, n1, p->nb, 0);
  return true;
}

size_t rdyn_tsqr_workspace_bytes(int n_cols_with_rhs)
{
  TsqrRowsPlan p;
  return tsqr_rows_plan(n_cols_with_rhs, &p) ? p.L.total_doubles * sizeof(double) : 0;
}

int rdyn_tsqr(const double* A, int64_t rows, int64_t lda, int n_cols, const double* bvec, double* R, int accumulate, void* workspace,
              size_t workspace_bytes, int device, void* stream_v)
{
  if (!A || !R || rows < 0 || lda < rows || n_cols < 1 || !workspace)
  {
    rdyn_set_error("rdyn_tsqr: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  const int n1 = n_cols + (bvec ? 1 : 0);
  TsqrRowsPlan p;
  if (!tsqr_rows_plan(n1, &p))
  {
    rdyn_set_error("rdyn_tsqr: at most %d columns (right-hand side included) are supported", rdyn_tsqr_wide_max_cols());
    return RDYN_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < p.L.total_doubles * sizeof(double))
  {
    rdyn_set_error("rdyn_tsqr: workspace too small");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g;
  int st = g.enter(device);
  if (st != RDYN_OK) return st;
  hipStream_t stream = (hipStream_t)stream_v;
  if (rows == 0)
  {
    if (!accumulate) RDYN_HIP_TRY(hipMemsetAsync(R, 0, sizeof(double) * n1 * n1, stream));
    return RDYN_OK;
  }
  double* const ws = (double*)workspace;
  const TsqrLayout& L = p.L;
  // the Householder folds of all rows: in registers up to 64 columns, with the factor in LDS beyond
  auto householder = [&](double* R_to, int acc, const int* run_flag, int fan) -> int {
    if (p.nc_reg)
    {
      const int64_t blocks64 = (rows + 63) / 64;  // one wave folds 64 rows at a time
      const int blocks = (int)((blocks64 + 3) / 4 < kTsqrBlocks ? (blocks64 + 3) / 4 : kTsqrBlocks);
      RDYN_HIP_TRY(rdyn_launch_tsqr_rows(A, bvec, rows, lda, n_cols, blocks, ws, R_to, acc, stream, run_flag, fan));
    }
    else
      RDYN_HIP_TRY(rdyn_launch_tsqr_wide_rows(A, bvec, rows, lda, n_cols, kTsqrBlocks, ws, R_to, acc, run_flag, stream));
    return RDYN_OK;
  };
  const int64_t groups = (rows + 15) / 16;
  const bool cholqr = p.cholqr_ok && groups >= kCholqrMinGroups;
  if (!cholqr) return householder(R, accumulate ? 1 : 0, nullptr, 2);
  // ---- preconditioned CholeskyQR on the matrix cores (rdyn_cholqr.hip), as the fused routes below: the Gram matrix of every S-th
  // 16-row group (about 8 192 groups), the rounds, the stand-by
  const int64_t kSubGroups = 8192;
  int64_t gs = groups / kSubGroups > 1 ? groups / kSubGroups : 1;
  if (gs > 1 && gs % 2 == 0) ++gs;  // odd: does not lock onto power-of-two periods of the rows
  const int64_t sub_groups = (groups + gs - 1) / gs;
  int* const flag = (int*)(ws + L.flag);
  {
    RdynGramArgs sa;
    memset(&sa, 0, sizeof sa);
    // [A | b] as ONE matrix of n1 columns whose last column is split off as the right-hand side of the dense steps
    sa.A = A;
    sa.b = bvec ? bvec : A + (int64_t)(n1 - 1) * lda;
    sa.rows = rows;
    sa.lda = lda;
    sa.P = n1 - 1;
    sa.slabs = ws + L.slabs;
    sa.G = ws + L.g2;
    sa.c = ws + L.g2 + (size_t)(n1 - 1) * (n1 - 1);
    sa.bb = sa.c + (n1 - 1);
    sa.group_stride = (int)gs;
    const int sub4 = (int)((sub_groups + 3) / 4 < kCholqrBlocks ? (sub_groups + 3) / 4 : kCholqrBlocks);
    RDYN_HIP_TRY(rdyn_launch_gram(sa, sub4, stream));
    RDYN_HIP_TRY(rdyn_launch_gram_finish(sa, sub4, stream));
  }
  double* const R_new = accumulate ? ws + L.r_swept : R;
  const int blocks = (int)((groups + 3) / 4 < kCholqrBlocks ? (groups + 3) / 4 : kCholqrBlocks);
  st = cholqr_rounds(ws, L, n1, 0, p.nb, p.nb, 1, sqrt((double)groups / (double)sub_groups), blocks, R_new, stream,
                     [&](const double* W, const int* run, double* slabs) -> int {
                       RDYN_HIP_TRY(rdyn_launch_pgram_rows(A, bvec, rows, lda, n_cols, W, slabs, run, blocks, stream));
                       return RDYN_OK;
                     });
  if (st != RDYN_OK) return st;
  st = householder(R_new, 0, flag + 1, 16);  // stand-by: started by the device only when neither round was accepted
  if (st != RDYN_OK) return st;
  if (accumulate) RDYN_HIP_TRY(rdyn_launch_cholqr_fold(R_new, R, n1, stream));
  return RDYN_OK;
}

int rdyn_tsqr_rows_last_report(int n_cols_with_rhs, int64_t rows, const void* workspace, int device, void* stream, rdyn_tsqr_report* out)
{
  TsqrRowsPlan p;
  if (!workspace || !out || rows < 0 || !tsqr_rows_plan(n_cols_with_rhs, &p))
  {
    rdyn_set_error("rdyn_tsqr_rows_last_report: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  memset(out, 0, sizeof *out);
  if (!p.cholqr_ok || (rows + 15) / 16 < kCholqrMinGroups) return RDYN_OK;  // route 0: the Householder folds, nothing to report
  DeviceGuard g;
  int st = g.enter(device);
  if (st != RDYN_OK) return st;
  double raw[96];
  RDYN_HIP_TRY(hipMemcpyAsync(raw, (const double*)workspace + p.L.flag, sizeof raw, hipMemcpyDeviceToHost, (hipStream_t)stream));
  RDYN_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  read_report(raw, p.n1, out);
  return RDYN_OK;
}

// ---- rdyn_regressor_tsqr / rdyn_identification_tsqr: rows generated by the sweep, never stored
// the chain whose rows are swept: the reduced companion when the chain has non-input joints (component columns belong to input
// joints, which the companion keeps in the same order: they ride along unchanged).  A companion of ONE joint is below what the
// sweeping kernels are built for: such a chain is swept as it is.

// rectangular 16-sample tile of rdyn_tsqr_wide.hip: every column 16 n rows + 4 doubles, structural zeros stored
static bool build_rect_tile(const rdyn_chain* c, int n_comp_cols, RdynLdsGramArgs* la)
{
  const int n = c->n_active(), nJ = c->n_joints();
  const int cs = (16 * n + 4) * 8;
  bool monotonic = true;
  for (int j = 1; j < n; ++j) monotonic = monotonic && c->active[j] > c->active[j - 1];
  la->all_revolute = 0;
  for (int f = 0; f < nJ; ++f)
  {
    int m = 0;
    for (int j = 0; j < n; ++j) m += (c->active[j] <= f) ? 1 : 0;
    la->lds_m[f] = m;
    la->lds_stride[f] = cs;
    la->lds_off[f] = 10 * f * cs;
  }
  la->lds_off_c = 10 * nJ * cs;
  la->comp_stride = cs;
  la->comp_row_step = 128;
  la->lds_off_b = (10 * nJ + n_comp_cols) * cs;
  la->tile_bytes = (10 * nJ + n_comp_cols + 1) * cs;
  la->n_active = n;
  for (int j = 0; j < n; ++j) la->first_col[j] = 10 * c->active[j];
  fill_in_map(c, la);
  return monotonic;
}

// everything a factor call decides from (chain, components) alone: which chain is swept, which kernels serve it, the workspace
struct TsqrPlan
{
  const rdyn_chain* cs = nullptr;
  bool expand = false;
  int n = 0, nJ = 0, K = 0, xb = 0;
  int n1s = 0, n1 = 0;        // factor widths: swept chain, chain
  int nc_reg = 0;             // padded factor width of the register-resident folds of rdyn_tsqr.hip (0: they do not serve the shape)
  bool wide = false;          // the LDS-resident folds of rdyn_tsqr_wide.hip serve the shape
  int pairs = 0, nb = 0;      // preconditioned route: pass-B configuration (0: not served), 16-column blocks of its column space
  bool sub_compact = false;   // the subsample pass (four tiles per workgroup) needs the compact tile
  // 9 .. 10 input joints (more rows per sample than the tile kernels' sweepers hold): the rows go through a chunk image in the
  // workspace -- swept by the one-thread-per-sample kernel, factored by rdyn_tsqr's kernels, chunk after chunk
  bool image = false;
  bool long_image = false;    // ... of a chain with 11 input joints (no companion): the chunk image comes from rdyn_long_local.hip
  size_t img_off = 0, rows_off = 0;  // doubles: the chunk image, rdyn_tsqr's own workspace
  RdynLdsGramArgs la, la_sub, la_wide;
  RdynLdsGramArgs la_b;       // pass B's tile: la, or the layout of the one-lane-per-sample sweepers (sweep_lanes set)
  TsqrLayout L;
  const char* why = nullptr;  // when nothing serves the shape
};

static bool tsqr_plan(const rdyn_chain* c, const rdyn_component* comps, int n_comps, TsqrPlan* p)
{
  // the chain whose rows are swept: the reduced companion where the chain has joints that are not input joints; the tile kernels sweep
  // its sorted view (input joints listed out of chain order)
  const rdyn_chain* const raw = (c->reduced && c->reduced->n_joints() >= 2) ? c->reduced.get() : c;
  p->cs = ordered(raw);
  p->expand = raw != c;
  if (c->long_chain() && !p->expand)
  {
    // no companion (more than 10 input joints): served as long as the factor fits the widest one the kernels hold -- 11 input joints
    // without component columns (110 + 1 columns) -- through chunk images of the run-time-length regressor kernel
    const int K0 = n_comps > 0 ? rdyn_components_columns(comps, n_comps) : 0;
    if (K0 != 0 || 10 * c->n_joints() + 1 > rdyn_tsqr_wide_max_cols() || c->n_active() != c->n_joints())
    {
      p->why = "a chain of more than 10 joints needs 2 .. 10 input joints (11 without fixed joints and component columns)";
      return false;
    }
    p->cs = c;
    p->n = c->n_active();
    p->nJ = c->n_joints();
    p->K = 0;
    p->xb = 0;
    p->n1s = p->n1 = 10 * p->nJ + 1;
    memset(&p->la, 0, sizeof p->la);
    memset(&p->la_sub, 0, sizeof p->la_sub);
    memset(&p->la_wide, 0, sizeof p->la_wide);
    memset(&p->la_b, 0, sizeof p->la_b);
    p->image = p->long_image = true;
    p->L = tsqr_layout(0, p->n1s, 0, 0);
    p->img_off = (p->L.total_doubles + 31) & ~(size_t)31;
    p->rows_off = p->img_off + (size_t)kTsqrImageChunk * p->n * p->n1s;
    p->L.total_doubles = p->rows_off + rdyn_tsqr_workspace_bytes(p->n1s) / sizeof(double);
    return true;
  }
  const rdyn_chain* cs = p->cs;
  p->n = cs->n_active();
  p->nJ = cs->n_joints();
  const int K = n_comps > 0 ? rdyn_components_columns(comps, n_comps) : 0;
  if (K < 0 || K > 96)
  {
    p->why = "invalid components";
    return false;
  }
  p->K = K;
  p->xb = K > 0 ? 1 : 0;
  p->n1s = 10 * p->nJ + K + 1;
  p->n1 = 10 * c->n_joints() + K + 1;
  memset(&p->la, 0, sizeof p->la);
  memset(&p->la_sub, 0, sizeof p->la_sub);
  memset(&p->la_wide, 0, sizeof p->la_wide);
  memset(&p->la_b, 0, sizeof p->la_b);
  if (p->n > 8 && p->n <= RDYN_MAX_SWEPT_JOINTS && p->n == p->nJ && p->n1s <= rdyn_tsqr_wide_max_cols() &&
      !(p->expand && rdyn_cholqr_expand_lds_bytes(c->n_joints(), p->nJ, K) > 156 * 1024))
  {
    p->image = true;
    p->cs = raw;  // (the image's rows are the caller's input indices: the one-thread-per-sample sweep and the component kernel agree on that)
    p->L = tsqr_layout(0, p->n1s, 0, p->expand ? p->n1 : 0);
    p->img_off = (p->L.total_doubles + 31) & ~(size_t)31;
    p->rows_off = p->img_off + (size_t)kTsqrImageChunk * p->n * p->n1s;
    p->L.total_doubles = p->rows_off + rdyn_tsqr_workspace_bytes(p->n1s) / sizeof(double);
    return true;
  }
  if (p->n < 1 || p->n > 8 || p->nJ < 1 || !build_rect_tile(cs, K, &p->la_wide))
  {
    p->why = "chains of 1..10 input joints whose factor (after the reduction) has at most 112 columns are supported";
    return false;
  }
  const bool tile_ok = build_lds_tile(cs, K, &p->la) && 4 * (size_t)p->la.tile_bytes <= 160 * 1024;
  // register-resident Householder folds: 2..7 joints, 2..6 with component columns (which must fit one 16-column slot)
  p->nc_reg = (tile_ok && p->nJ >= 2 && p->nJ <= 7) ? rdyn_regressor_tsqr_cols(p->nJ, K) : 0;
  // LDS-resident folds: the rectangular tile beside the packed factor
  p->wide = rdyn_regressor_tsqr_wide_lds_bytes(p->n1s, p->n) != 0;
  // preconditioned route: every joint of the swept chain an input joint, the factor within the dense kernels' LDS, the component
  // columns within the one extra column block, and a subsample kernel for the shape
  p->nb = (10 * p->nJ + 1 + 15) / 16 + p->xb;
  if (p->n == p->nJ && p->nJ >= 2 && p->nJ <= 7 && p->n1s <= rdyn_cholqr_max_cols_lds() && p->n1s <= 16 * p->nb &&
      (K == 0 || rdyn_regressor_gram_duo_supports_components(10 * p->nJ, K)) && build_lds_tile(cs, K, &p->la))
  {
    p->pairs = rdyn_cholqr_pairs(p->nJ, p->la.tile_bytes, p->xb);
    if (p->pairs == -1)
    {
      // every wave sweeps and consumes its own COMPACT tile (k_regressor_pgram_solo): four of them fill the LDS, W stays in global memory
      RdynLdsGramArgs compact;
      memset(&compact, 0, sizeof compact);
      build_lds_tile(cs, K, &compact, true);
      if (4 * (size_t)compact.tile_bytes <= 160 * 1024)
        p->la = compact;
      else
        p->pairs = rdyn_cholqr_pairs(p->nJ, -p->la.tile_bytes, p->xb);  // too many component columns: two pairs beside W, or nothing
    }
    p->la_b = p->la;
    const int kin_pad = rdyn_cholqr_kin_pad(p->nJ, p->xb, p->pairs);
    if (kin_pad)
    {
      // one lane per sample: wave 0 the link kinematics, three row waves (7 joints: four compact tiles + the exchange area, W in global memory)
      RdynLdsGramArgs kin;
      memset(&kin, 0, sizeof kin);
      build_lds_tile(cs, K, &kin, kin_pad == 2);
      const size_t need = (p->pairs == 4 ? rdyn_cholqr_w_doubles(p->nJ, p->xb) * 8 : 0) + 4 * (size_t)kin.tile_bytes + RDYN_KIN_XCH_BYTES_XV(p->nJ <= 6 ? 21 : 12);
      if (need <= 160 * 1024)
      {
        fill_sw_rows(&kin, p->n, 3, 3, -1);
        kin.sweep_lanes = 1;
        p->la_b = kin;
      }
    }
    if (p->pairs != 0)
    {
      build_lds_tile(cs, K, &p->la_sub);
      if (4 * (size_t)p->la_sub.tile_bytes > 160 * 1024)
      {
        build_lds_tile(cs, K, &p->la_sub, true);
        p->sub_compact = true;
        if (4 * (size_t)p->la_sub.tile_bytes > 160 * 1024) p->pairs = 0;
      }
    }
  }
  if (!p->nc_reg && !p->wide)
  {
    p->why = "the factor does not fit the LDS-resident folds (at most 112 columns)";
    return false;
  }
  if (p->expand && rdyn_cholqr_expand_lds_bytes(c->n_joints(), p->nJ, K) > 156 * 1024)
  {
    p->why = "the expansion of the reduced chain's factor exceeds the LDS of one workgroup";
    return false;
  }
  size_t hh = p->wide ? rdyn_tsqr_wide_workspace_doubles(p->n1s, kTsqrBlocks) : 0;
  int n1w = p->n1s;
  if (p->nc_reg)
  {
    const size_t reg = rdyn_tsqr_workspace_doubles(p->nc_reg, kTsqrBlocks);
    if (reg > hh) hh = reg;
    if (p->nc_reg > n1w) n1w = p->nc_reg;
  }
  p->L = tsqr_layout(hh, n1w, p->pairs != 0 ? p->nb : 0, p->expand ? p->n1 : 0);
  return true;
}

// [A C b] = [A_red C b] diag(E, I_K, 1): R = qr(R_swept diag(E, I_K, 1)), folded into the caller's factor through `scratch` (n1 x n1
// doubles) when accumulating
static int expand_factor(const rdyn_chain* c, const TsqrPlan& p, const double* R_swept, double* R, int accumulate, double* scratch, hipStream_t stream)
{
  RdynGramExpandArgs ea;
  int st = fill_expand_args(c, p.nJ, p.K, &ea);
  if (st != RDYN_OK) return st;
  double* const R_exp = accumulate ? scratch : R;
  RDYN_HIP_TRY(rdyn_launch_cholqr_expand(ea, R_swept, R_exp, stream));
  if (accumulate) RDYN_HIP_TRY(rdyn_launch_cholqr_fold(R_exp, R, p.n1, stream, p.n1s));
  return RDYN_OK;
}

// swept_only: stop at the factor of the SWEPT chain (n1s x n1s into R, no expansion, no accumulation): the multi-device form gathers
// and folds these -- the smaller payload, and no limit on the width of the expanded factor -- and expands once per device
static int regressor_tsqr_run(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b, const double* tau_meas, double* R,
                              int accumulate, void* workspace, size_t workspace_bytes, const char* who, bool swept_only = false)
{
  // (a long chain without a companion: tsqr_plan decides -- 11 input joints are served through chunk images)
  int st = check_batch(c, b, true, true, who, (c && c->long_chain() && !c->reduced) ? LONG_KERNELS : LONG_COMPANION);
  if (st != RDYN_OK) return st;
  if (!R || !workspace || n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps))
  {
    rdyn_set_error("%s: null output / workspace, or more than %d components", who, RDYN_MAX_COMPONENTS);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  TsqrPlan p;
  if (!tsqr_plan(c, comps, n_comps, &p))
  {
    rdyn_set_error("%s: %s", who, p.why);
    return RDYN_ERR_UNSUPPORTED;
  }
  const rdyn_chain* cs = p.cs;  // chains with fixed joints: the reduced companion is swept, the factor expanded
  const bool expand = p.expand && !swept_only;
  if (swept_only) accumulate = 0;
  const int n = p.n, nJ = p.nJ, K = p.K, n1s = p.n1s, n1 = p.n1;
  const TsqrLayout& L = p.L;
  if (workspace_bytes < L.total_doubles * sizeof(double))
  {
    rdyn_set_error("%s: workspace too small", who);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  RdynComponentArgs ca;
  memset(&ca, 0, sizeof ca);
  if (n_comps > 0)
  {
    st = fill_components(comps, n_comps, n, &ca);
    if (st != RDYN_OK) return st;
  }
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  const RdynChainConst* dc = nullptr;
  const RdynLongChainConst* dcl = nullptr;
  st = p.long_image ? device_const_long(cs, &dcl) : device_const(cs, &dc);
  if (st != RDYN_OK) return st;
  hipStream_t stream = (hipStream_t)b->stream;
  if (b->n_samples == 0)
  {
    if (!accumulate) RDYN_HIP_TRY(hipMemsetAsync(R, 0, sizeof(double) * (swept_only ? (size_t)n1s * n1s : (size_t)n1 * n1), stream));
    return RDYN_OK;
  }
  if (p.image)
  {
    // ---- 9 .. 10 input joints: [Y | C | tau_meas] of a chunk as an element-major image (rows j * cnt + s), factored by rdyn_tsqr's
    // kernels (matrix cores up to 96 columns, LDS-resident Householder folds beyond) and folded into the running factor
    double* const ws = (double*)workspace;
    double* const img = ws + p.img_off;
    double* const R_swept = expand ? ws + L.r_swept : R;
    const int cols = n1s - 1;  // columns in front of the right-hand side
    // (11 input joints: the image by the run-time-length kernel)
    ChunkImage im(cs, b, tau_meas, img, cols, &ca, n_comps, K);
    im.dc = dc;
    im.dl = dcl;
    for (int64_t s0 = 0; s0 < b->n_samples; s0 += kTsqrImageChunk)
    {
      const int64_t cnt = (b->n_samples - s0 < kTsqrImageChunk) ? (b->n_samples - s0) : kTsqrImageChunk;
      st = im.write(s0, cnt, 1, stream);
      if (st != RDYN_OK) return st;
      // (without measured torques the image's last column stays zero: the factor of [A | 0])
      st = rdyn_tsqr(img, (int64_t)n * cnt, (int64_t)n * cnt, cols, img + (int64_t)cols * n * cnt, R_swept, (s0 > 0 || (accumulate && !expand)) ? 1 : 0,
                     ws + p.rows_off, rdyn_tsqr_workspace_bytes(n1s), -1, stream);
      if (st != RDYN_OK) return st;
    }
    return expand ? expand_factor(c, p, R_swept, R, accumulate, ws + L.r_full, stream) : RDYN_OK;
  }
  auto bind = [&](RdynLdsGramArgs& la) {
    la.chain = dc;
    la.q = b->q;
    la.dq = b->dq;
    la.ddq = b->ddq;
    la.bcol = tau_meas;
    la.n_samples = b->n_samples;
    rec_strides(b, n, &la.in_ss, &la.in_sj);
    la.n_comps = n_comps;
    la.n_comp_cols = K;
    int col = 0;
    for (int i = 0; i < n_comps; ++i)
    {
      la.comps[i] = ca.comps[i];
      la.comps[i].joint = cs->input_row[ca.comps[i].joint];  // the tile row of the component's input joint (sorted view)
      const int w = ca.comps[i].type == RDYN_COMP_FRICTION2 ? 3 : 2;
      for (int k = 0; k < w; ++k) la.comp_col_row[col++] = (signed char)la.comps[i].joint;
    }
  };
  bind(p.la);
  bind(p.la_b);
  bind(p.la_sub);
  bind(p.la_wide);
  double* const ws = (double*)workspace;
  const int64_t tiles = (b->n_samples + 15) / 16;
  // the Householder folds of all rows: rdyn_tsqr.hip where the factor fits a wave's registers, rdyn_tsqr_wide.hip otherwise
  auto householder = [&](double* R_to, int acc, const int* run_flag, int fan) -> int {
    if (p.nc_reg)
    {
      RdynLdsGramArgs all = p.la;
      all.run_flag = run_flag;
      const int hblocks = (int)((tiles + 3) / 4 < kTsqrBlocks ? (tiles + 3) / 4 : kTsqrBlocks);
      RDYN_HIP_TRY(rdyn_launch_regressor_tsqr(nJ, all, hblocks, 4 * (size_t)p.la.tile_bytes, ws, R_to, acc, stream, fan));
    }
    else
    {
      RdynLdsGramArgs all = p.la_wide;
      all.run_flag = run_flag;
      const int hblocks = (int)(tiles < kTsqrBlocks ? tiles : kTsqrBlocks);
      RDYN_HIP_TRY(rdyn_launch_regressor_tsqr_wide(nJ, all, hblocks, ws, R_to, acc, stream));
    }
    return RDYN_OK;
  };
  // ---- which route.  Preconditioned CholeskyQR (rdyn_cholqr.hip: the heavy pass on the matrix cores) for large batches of chains
  // whose swept form has every joint as an input joint; the Householder folds otherwise.
  const int pairs = p.pairs;
  const bool cholqr = pairs != 0 && tiles >= kCholqrMinTiles;
  // where the factor of the swept chain goes: straight into R when nothing follows
  double* const R_swept = (expand || (cholqr && accumulate)) ? ws + L.r_swept : R;
  if (cholqr)
  {
    // pass A: the Gram matrix of every S-th tile (about 1 024 tiles whatever the batch size: one tile per wave pair of the regressor ->
    // Gram kernel; 16 384 samples = 115 000 rows for <= 96 columns put the pivots of the second factorisation within a few % of 1).
    // A preconditioner does not have to be a backward-stable factor -- what it is worth is measured on all rows afterwards.
    RdynLdsGramArgs& la = p.la_b;
    RdynLdsGramArgs sub = p.la_sub;
    const int64_t kSubTiles = 1024;
    sub.tile_stride = (int)(tiles / kSubTiles > 1 ? tiles / kSubTiles : 1);
    if (sub.tile_stride > 1 && sub.tile_stride % 2 == 0) ++sub.tile_stride;  // odd: does not lock onto power-of-two periods of a trajectory
    const int64_t sub_tiles = (tiles + sub.tile_stride - 1) / sub.tile_stride;
    la.slabs = ws + L.slabs;
    sub.slabs = la.slabs;
    const int np = pairs == -1 ? 4 : (pairs < 0 ? -pairs : pairs);  // tiles a workgroup works on at a time
    const int blocks = (int)((tiles + np - 1) / np < kCholqrBlocks ? (tiles + np - 1) / np : kCholqrBlocks);
    int* const flag = (int*)(ws + L.flag);
    const int col_shift = pairs == -1 ? rdyn_cholqr_solo_col_shift(nJ, K) : rdyn_cholqr_col_shift(nJ, p.xb);
    la.col_shift = col_shift;
    {
      // the plain regressor -> Gram kernel (rdyn_duo_gram.hip) on the subsample: its slab layout (descending link order, component
      // columns in front), its workgroups of four pairs
      const int sub4 = (int)((sub_tiles + 3) / 4 < kCholqrBlocks ? (sub_tiles + 3) / 4 : kCholqrBlocks);
      const int nbt = p.nb;
      size_t lds_bytes = 4 * (size_t)sub.tile_bytes;
      const size_t red_bytes = (size_t)(nbt * (nbt + 1) / 2) * 256 * sizeof(double);
      if (lds_bytes < red_bytes) lds_bytes = red_bytes;
      RDYN_HIP_TRY(rdyn_launch_regressor_gram_duo(10 * nJ, sub, sub4, lds_bytes, stream));
      RdynGramArgs gs;
      memset(&gs, 0, sizeof gs);
      gs.P = n1s - 1;
      gs.slabs = la.slabs;
      gs.G = ws + L.g2;
      gs.c = ws + L.g2 + (size_t)(n1s - 1) * (n1s - 1);
      gs.bb = gs.c + (n1s - 1);
      gs.desc_nj = nJ;
      gs.desc_k = K;
      gs.slab_nb = K > 0 ? nbt : 0;
      RDYN_HIP_TRY(rdyn_launch_gram_finish(gs, sub4, stream));
    }
    st = cholqr_rounds(ws, L, n1s, col_shift, p.nb, K > 0 ? p.nb : 0, tau_meas ? 1 : 0, sqrt((double)tiles / (double)sub_tiles), blocks, R_swept, stream,
                       [&](const double* W, const int* run, double*) -> int {
                         RDYN_HIP_TRY(rdyn_launch_regressor_pgram(nJ, la, W, run, blocks, pairs, stream));
                         return RDYN_OK;
                       });
    if (st != RDYN_OK) return st;
    // stand-by: the Householder factorisation of ALL rows, queued behind the two rounds and started by the device only when a
    // preconditioner was unfit (growth factor) or round 1 was not accepted either (flag[1]; launches that leave at once otherwise).
    // It asks nothing of the batch, so the call as a whole is as robust as the Householder route whatever the subsample looked like.
    st = householder(R_swept, 0, flag + 1, 16);
    if (st != RDYN_OK) return st;
    if (!expand && accumulate) RDYN_HIP_TRY(rdyn_launch_cholqr_fold(R_swept, R, n1s, stream));
  }
  else
  {
    st = householder(R_swept, (accumulate && !expand) ? 1 : 0, nullptr, 2);
    if (st != RDYN_OK) return st;
  }
  return expand ? expand_factor(c, p, R_swept, R, accumulate, ws + L.r_full, stream) : RDYN_OK;
}

// ---- the pieces of a factor call the multi-device form (rdyn_multi_gpu.cpp) needs separately (C++ linkage, not exported)
__attribute__((visibility("hidden"))) int rdyn_internal_tsqr_widths(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int* n1s, int* n1, int* expands)
{
  TsqrPlan p;
  if (!c || !tsqr_plan(c, comps, n_comps, &p)) return RDYN_ERR_UNSUPPORTED;
  *n1s = p.n1s;
  *n1 = p.n1;
  *expands = p.expand ? 1 : 0;
  return RDYN_OK;
}
__attribute__((visibility("hidden"))) int rdyn_internal_tsqr_swept(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b,
                                                                   const double* tau_meas, double* R_swept, void* workspace, size_t workspace_bytes)
{
  return regressor_tsqr_run(c, comps, n_comps, b, tau_meas, R_swept, 0, workspace, workspace_bytes, "rdyn_identification_tsqr_multi", true);
}
// R <- (accumulate ? qr([R ; .]) : .) of  R_swept diag(E, I_K, 1);  scratch: n1 x n1 doubles (used when accumulating); current device
__attribute__((visibility("hidden"))) int rdyn_internal_tsqr_expand(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const double* R_swept,
                                                                    double* R, int accumulate, double* scratch, void* stream_v)
{
  TsqrPlan p;
  if (!tsqr_plan(c, comps, n_comps, &p) || !p.expand) return RDYN_ERR_UNSUPPORTED;
  return expand_factor(c, p, R_swept, R, accumulate, scratch, (hipStream_t)stream_v);
}

size_t rdyn_regressor_tsqr_workspace_bytes(const rdyn_chain* c)
{
  if (!c) return 0;
  TsqrPlan p;
  return tsqr_plan(c, nullptr, 0, &p) ? p.L.total_doubles * sizeof(double) : 0;
}

int rdyn_regressor_tsqr(const rdyn_chain* c, const rdyn_batch* b, const double* tau_meas, double* R, int accumulate, void* workspace,
                        size_t workspace_bytes)
{
  return regressor_tsqr_run(c, nullptr, 0, b, tau_meas, R, accumulate, workspace, workspace_bytes, "rdyn_regressor_tsqr");
}

size_t rdyn_identification_tsqr_workspace_bytes(const rdyn_chain* c, const rdyn_component* comps, int n_comps)
{
  if (!c || n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps)) return 0;
  TsqrPlan p;
  return tsqr_plan(c, comps, n_comps, &p) ? p.L.total_doubles * sizeof(double) : 0;
}

int rdyn_identification_tsqr(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b, const double* tau_meas, double* R,
                             int accumulate, void* workspace, size_t workspace_bytes)
{
  return regressor_tsqr_run(c, comps, n_comps, b, tau_meas, R, accumulate, workspace, workspace_bytes, "rdyn_identification_tsqr");
}

int rdyn_tsqr_last_report(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int64_t n_samples, const void* workspace, int device,
                          void* stream, rdyn_tsqr_report* out)
{
  if (!c || !workspace || !out || n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps) || n_samples < 0)
  {
    rdyn_set_error("rdyn_tsqr_last_report: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  memset(out, 0, sizeof *out);
  TsqrPlan p;
  if (!tsqr_plan(c, comps, n_comps, &p))
  {
    rdyn_set_error("rdyn_tsqr_last_report: the factor entry points do not serve this chain");
    return RDYN_ERR_UNSUPPORTED;
  }
  if (p.image || p.pairs == 0 || (n_samples + 15) / 16 < kCholqrMinTiles) return RDYN_OK;  // route 0: the Householder folds, nothing to report
  DeviceGuard g;
  int st = g.enter(device);
  if (st != RDYN_OK) return st;
  double raw[96];
  RDYN_HIP_TRY(hipMemcpyAsync(raw, (const double*)workspace + p.L.flag, sizeof raw, hipMemcpyDeviceToHost, (hipStream_t)stream));
  RDYN_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  read_report(raw, p.n1s, out);
  return RDYN_OK;
}


// ---- R factors wider than 112 columns: preconditioned CholeskyQR over column panels (rdyn_panel_trmm.hip, rdyn_panel_gram.hip and
// the PANEL instantiations of rdyn_cholqr.hip's dense steps).  Round 0: W from the Gram matrix of a row subsample; round r = 1, 2: W from
// round r - 1's factor, started by the device when the round before was not accepted.  Per round: Q = [A b] W (k_panel_trmm), Q'Q
// (k_panel_gram over every chunk + finish), R = chol(Q'Q) T.  Nothing falls back to Householder folds: they do not exist beyond 112 columns.
// Workspace: [flags | slabs | W | T | V | G2 | R_tmp | squares | fold scratch | one row chunk of Q] -- the flags first, so that the
// report needs nothing but the workspace and the width.
static const int64_t kPanelQrRowBytes = (int64_t)128 << 20;  // rows region: 128 MiB (rdyn_tsqr_wide: one row chunk of Q)
static const int64_t kPanelQrMinRows = 16384;
static const int64_t kPanelQrSubGroups = 4096;     // rdyn_tsqr_wide's subsample: about 4 096 16-row groups
static const int64_t kPanelQrSubSamples = 16384;   // the chain forms: one chunk image of about 16 384 samples
static const int kPanelFlagDoubles = 256;          // ints [0..15] flags, [16 .. 16 + n1) deferred columns; doubles [224 + 4 r ..] diagnostics

struct PanelQrLayout
{
  size_t flag = 0, slabs = 0, w = 0, t = 0, v = 0, g2 = 0, r_tmp = 0, sq = 0, fold = 0, rows = 0, total_doubles = 0;
};
static PanelQrLayout panel_qr_layout(int n1, size_t rows_doubles)
{
  PanelQrLayout L;
  size_t off = 0;
  auto take = [&](size_t doubles) {
    const size_t at = off;
    off = (off + doubles + 31) & ~(size_t)31;
    return at;
  };
  const int nb = (n1 + 15) / 16, nt = nb * (nb + 1) / 2;
  L.flag = take(kPanelFlagDoubles);
  L.slabs = take(panel_slab_bytes(n1 - 1) / sizeof(double));
  L.w = take((size_t)nt * 256);
  L.t = take((size_t)n1 * n1);
  L.v = take((size_t)n1 * n1);
  L.g2 = take((size_t)n1 * n1 + 1);
  L.r_tmp = take((size_t)n1 * n1);
  L.sq = take((size_t)2 * n1 * n1);
  L.fold = take((size_t)n1 * (n1 + 1) / 2);
  L.rows = take(rows_doubles);
  L.total_doubles = off;
  return L;
}
static bool panel_qr_width_ok(int n1) { return n1 > rdyn_tsqr_wide_max_cols() && n1 <= RDYN_MAX_WIDE_COLUMNS + 1 && n1 <= rdyn_cholqr_panel_max_cols(); }
static int64_t panel_qr_q_rows(int n1)
{
  const int64_t fit = (kPanelQrRowBytes / ((int64_t)n1 * (int64_t)sizeof(double))) & ~(int64_t)63;
  return fit > kPanelQrMinRows ? fit : kPanelQrMinRows;
}

// the three rounds on the subsample Gram matrix in ws + L.g2; pass_b(W, run, round) queues Q = X W and Q'Q into L.g2 for all rows
typedef std::function<int(const double* W, const int* run, int round)> PanelPassB;
static int panel_qr_rounds(double* ws, const PanelQrLayout& L, int n1, int has_b, double row_scale, double* R_out, hipStream_t stream,
                           const PanelPassB& pass_b)
{
  int* const flag = (int*)(ws + L.flag);
  const int P = n1 - 1;
  double* const G = ws + L.g2;
  double* const c = G + (size_t)P * P;
  double* const bb = c + P;
  const int nb = (n1 + 15) / 16;
  for (int round = 0; round < 3; ++round)
  {
    const int* const run = round == 0 ? nullptr : flag + (round - 1);
    double* const diag = ws + L.flag + 224 + 4 * round;  // [0] rho, [1] gamma of the preconditioner, [2] gamma of the factor
    RDYN_HIP_TRY(rdyn_launch_cholqr_precond_panel(round == 0 ? nullptr : R_out, round == 0 ? G : nullptr, c, bb, n1, nb, round == 0 ? row_scale : 1.0,
                                                  ws + L.t, ws + L.w, ws + L.v, flag + 16, flag, round, run, diag + 1, ws + L.sq, stream));
    const int st = pass_b(ws + L.w, run, round);
    if (st != RDYN_OK) return st;
    RDYN_HIP_TRY(rdyn_launch_cholqr_factor_panel(G, c, bb, n1, has_b, ws + L.t, ws + L.v, flag + 16, R_out, flag, round, run, diag, ws + L.sq, stream));
  }
  return RDYN_OK;
}

static void read_wide_report(const double* raw, int n1, rdyn_tsqr_wide_report* out)
{
  int flags[2 * kPanelFlagDoubles];
  memcpy(flags, raw, sizeof flags);
  out->route = 2;
  out->stage = 3;
  for (int r = 2; r >= 0; --r)
    if (flags[4 + r] && !flags[8 + r]) out->stage = r;
  const int width = (flags[3] > 0 && flags[3] < n1) ? flags[3] : n1;  // (a chain with fixed joints: the companion's factor was computed)
  for (int k = 0; k < width && 16 + k < 2 * kPanelFlagDoubles; ++k) out->n_deferred += flags[16 + k] ? 1 : 0;
  for (int r = 0; r < 3; ++r)
    if (flags[4 + r])
    {
      out->rho[r] = raw[224 + 4 * r];
      out->gamma[r] = raw[224 + 4 * r + 2];
    }
}

size_t rdyn_tsqr_wide_workspace_bytes(int n_cols_with_rhs)
{
  const int n1 = n_cols_with_rhs;
  if (n1 >= 1 && n1 <= rdyn_tsqr_wide_max_cols()) return rdyn_tsqr_workspace_bytes(n1);
  if (!panel_qr_width_ok(n1)) return 0;
  return panel_qr_layout(n1, (size_t)panel_qr_q_rows(n1) * n1).total_doubles * sizeof(double);
}

int rdyn_tsqr_wide(const double* A, int64_t rows, int64_t lda, int n_cols, const double* bvec, double* R, int accumulate, void* workspace,
                   size_t workspace_bytes, int device, void* stream_v)
{
  if (!A || !R || rows < 0 || lda < rows || n_cols < 1 || !workspace)
  {
    rdyn_set_error("rdyn_tsqr_wide: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  const int n1 = n_cols + (bvec ? 1 : 0);
  if (n1 <= rdyn_tsqr_wide_max_cols()) return rdyn_tsqr(A, rows, lda, n_cols, bvec, R, accumulate, workspace, workspace_bytes, device, stream_v);
  if (!panel_qr_width_ok(n1))
  {
    rdyn_set_error("rdyn_tsqr_wide: at most %d columns (right-hand side included) are supported", RDYN_MAX_WIDE_COLUMNS + 1);
    return RDYN_ERR_UNSUPPORTED;
  }
  const int64_t q_rows = panel_qr_q_rows(n1);
  const PanelQrLayout L = panel_qr_layout(n1, (size_t)q_rows * n1);
  if (workspace_bytes < L.total_doubles * sizeof(double))
  {
    rdyn_set_error("rdyn_tsqr_wide: workspace too small (%zu < %zu bytes)", workspace_bytes, L.total_doubles * sizeof(double));
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g;
  int st = g.enter(device);
  if (st != RDYN_OK) return st;
  hipStream_t stream = (hipStream_t)stream_v;
  if (rows == 0)
  {
    if (!accumulate) RDYN_HIP_TRY(hipMemsetAsync(R, 0, sizeof(double) * n1 * n1, stream));
    return RDYN_OK;
  }
  double* const ws = (double*)workspace;
  double* const Q = ws + L.rows;
  // [A | b] as ONE matrix of n1 columns (the last one the right-hand side of the dense steps, as in rdyn_tsqr)
  const int nA = bvec ? n_cols : n_cols - 1;
  const double* const bcol = bvec ? bvec : A + (int64_t)(n1 - 1) * lda;
  // pass A: every gs-th 16-row group (odd gs: no lock onto power-of-two periods of the rows), at most one row chunk
  const int64_t groups = (rows + 15) / 16;
  int64_t gs = groups / kPanelQrSubGroups > 1 ? groups / kPanelQrSubGroups : 1;
  if (gs > 1 && gs % 2 == 0) ++gs;
  while (rdyn_panel_gather_rows(rows, gs) > q_rows) gs += 2;
  const int64_t sub_rows = rdyn_panel_gather_rows(rows, gs);
  const int P = n1 - 1;  // Q'Q of [Q | b] goes to L.g2: G (P x P) | c | bb
  double* const G2 = ws + L.g2;
  double* const c2 = G2 + (size_t)P * P;
  RDYN_HIP_TRY(rdyn_launch_panel_gather(A, bcol, rows, lda, nA, gs, Q, q_rows, stream));
  st = panel_gram_launch(Q, sub_rows, q_rows, P, Q + (int64_t)P * q_rows, G2, c2, c2 + P, 0, true, 0, ws + L.slabs, nullptr, stream);
  if (st != RDYN_OK) return st;
  double* const R_new = accumulate ? ws + L.r_tmp : R;
  const double row_scale = sqrt((double)groups * 16.0 / (double)sub_rows);
  st = panel_qr_rounds(ws, L, n1, 1, row_scale, R_new, stream, [&](const double* W, const int* run, int) -> int {
    for (int64_t r0 = 0; r0 < rows; r0 += q_rows)
    {
      const int64_t cnt = rows - r0 < q_rows ? rows - r0 : q_rows;
      RdynPanelTrmmArgs ta;
      memset(&ta, 0, sizeof ta);
      ta.A = A + r0;
      ta.b = bcol + r0;
      ta.rows = cnt;
      ta.lda = lda;
      ta.n_cols = nA;
      ta.n1 = n1;
      ta.Q = Q;
      ta.ldq = q_rows;
      ta.W = W;
      ta.run_flag = run;
      RDYN_HIP_TRY(rdyn_launch_panel_trmm(ta, stream));
      const int s2 = panel_gram_launch(Q, cnt, q_rows, P, Q + (int64_t)P * q_rows, G2, c2, c2 + P, r0 > 0, r0 + cnt >= rows, 0, ws + L.slabs, run, stream);
      if (s2 != RDYN_OK) return s2;
    }
    return RDYN_OK;
  });
  if (st != RDYN_OK) return st;
  if (accumulate) RDYN_HIP_TRY(rdyn_launch_cholqr_fold_global(R_new, R, n1, ws + L.fold, stream));
  return RDYN_OK;
}

int rdyn_tsqr_wide_last_report(int n_cols_with_rhs, const void* workspace, int device, void* stream, rdyn_tsqr_wide_report* out)
{
  if (!workspace || !out || n_cols_with_rhs < 1)
  {
    rdyn_set_error("rdyn_tsqr_wide_last_report: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (n_cols_with_rhs > rdyn_tsqr_wide_max_cols() && !panel_qr_width_ok(n_cols_with_rhs))
  {
    rdyn_set_error("rdyn_tsqr_wide_last_report: at most %d columns are supported", RDYN_MAX_WIDE_COLUMNS + 1);
    return RDYN_ERR_UNSUPPORTED;
  }
  memset(out, 0, sizeof *out);
  if (n_cols_with_rhs <= rdyn_tsqr_wide_max_cols()) return RDYN_OK;  // route 0: served by rdyn_tsqr (rdyn_tsqr_rows_last_report)
  DeviceGuard g;
  int st = g.enter(device);
  if (st != RDYN_OK) return st;
  double raw[kPanelFlagDoubles];
  RDYN_HIP_TRY(hipMemcpyAsync(raw, workspace, sizeof raw, hipMemcpyDeviceToHost, (hipStream_t)stream));
  RDYN_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  read_wide_report(raw, n_cols_with_rhs, out);
  return RDYN_OK;
}

// chains: served by the narrow call where it serves (its workspace); else by chunk images of the chain itself -- [Y | C | tau_meas]
// written by ChunkImage, multiplied by W in place (k_panel_trmm), reduced by the panel Gram; a chain with
// fixed joints through its reduced companion (served by chunk images itself), whose factor is expanded by k_cholqr_expand<true>
// (R = qr(R_red E_aug)) -- the companion's workspace first (its flags are what the report reads), then R_red, the expansion's square,
// the expanded factor (accumulate) and the fold's triangle.
struct PanelQrPlan
{
  bool narrow = false, reduced = false;
  int K = 0, cols = 0, n1 = 0, n1r = 0;
  int64_t chunk = 0;
  size_t bytes = 0, sub_bytes = 0;
  PanelQrLayout L;
};
static PanelQrPlan panel_qr_plan(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int64_t chunk_samples, bool ident)
{
  PanelQrPlan p;
  if (!c || c->n_joints() < 1 || n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps) || chunk_samples < 0) return p;
  const size_t narrow = ident ? rdyn_identification_tsqr_workspace_bytes(c, comps, n_comps) : rdyn_regressor_tsqr_workspace_bytes(c);
  if (narrow > 0)
  {
    p.narrow = true;
    p.bytes = narrow;
    return p;
  }
  p.K = n_comps > 0 ? rdyn_components_columns(comps, n_comps) : 0;
  p.cols = 10 * c->n_joints() + p.K;
  p.n1 = p.cols + 1;
  if (!panel_qr_width_ok(p.n1)) return p;
  if (c->reduced)
  {
    const PanelQrPlan r = panel_qr_plan(c->reduced.get(), comps, n_comps, chunk_samples, ident);
    if (r.narrow || r.reduced || r.bytes == 0) return p;  // (a companion the narrow call serves: the narrow call serves the chain)
    p.reduced = true;
    p.n1r = r.n1;
    p.sub_bytes = align256(r.bytes);
    const size_t tail = (size_t)p.n1r * p.n1r + (size_t)p.n1 * p.n1r + (size_t)p.n1 * p.n1 + (size_t)p.n1 * (p.n1 + 1) / 2 + 128;
    p.bytes = p.sub_bytes + tail * sizeof(double);
    return p;
  }
  p.chunk = wide_chunk(c, p.cols, chunk_samples);
  p.L = panel_qr_layout(p.n1, (size_t)p.chunk * c->n_active() * p.n1);
  p.bytes = p.L.total_doubles * sizeof(double);
  return p;
}

static int panel_qr_chain_run(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b, const double* tau_meas, double* R,
                              int accumulate, int64_t chunk_samples, void* workspace, size_t workspace_bytes, bool ident)
{
  const char* fn = ident ? "rdyn_identification_tsqr_wide" : "rdyn_regressor_tsqr_wide";
  int st = check_batch(c, b, true, true, fn, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!R || !workspace || n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps) || chunk_samples < 0)
  {
    rdyn_set_error("%s: null output / workspace, negative chunk, or more than %d components", fn, RDYN_MAX_COMPONENTS);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  const int n = c->n_active();
  RdynComponentArgs ca;
  memset(&ca, 0, sizeof ca);
  st = fill_components(comps, n_comps, n, &ca);
  if (st != RDYN_OK) return st;
  const PanelQrPlan p = panel_qr_plan(c, comps, n_comps, chunk_samples, ident);
  if (p.bytes == 0)
  {
    rdyn_set_error("%s: this chain is not served (at most %d columns with the rhs; chains with fixed joints: the narrow limit)", fn,
                   RDYN_MAX_WIDE_COLUMNS + 1);
    return RDYN_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < p.bytes)
  {
    rdyn_set_error("%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes, p.bytes);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (p.narrow)
    return ident ? rdyn_identification_tsqr(c, comps, n_comps, b, tau_meas, R, accumulate, workspace, workspace_bytes)
                 : rdyn_regressor_tsqr(c, b, tau_meas, R, accumulate, workspace, workspace_bytes);
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  hipStream_t stream = (hipStream_t)b->stream;
  const int cols = p.cols, K = p.K, n1 = p.n1;
  const int64_t N = b->n_samples;
  if (N == 0)
  {
    if (!accumulate) RDYN_HIP_TRY(hipMemsetAsync(R, 0, sizeof(double) * n1 * n1, stream));
    return RDYN_OK;
  }
  if (p.reduced)
  {
    double* const R_red = (double*)((char*)workspace + p.sub_bytes);
    double* const B = R_red + (size_t)p.n1r * p.n1r;
    double* const R_exp = B + (size_t)n1 * p.n1r;
    double* const fold = R_exp + (size_t)n1 * n1;
    st = panel_qr_chain_run(c->reduced.get(), comps, n_comps, b, tau_meas, R_red, 0, chunk_samples, workspace, p.sub_bytes, ident);
    if (st != RDYN_OK) return st;
    RdynGramExpandArgs ea;
    st = fill_expand_args(c, c->reduced->n_joints(), K, &ea);
    if (st != RDYN_OK) return st;
    double* const R_out = accumulate ? R_exp : R;
    RDYN_HIP_TRY(rdyn_launch_cholqr_expand_global(ea, R_red, R_out, B, stream));
    if (accumulate) RDYN_HIP_TRY(rdyn_launch_cholqr_fold_global(R_exp, R, n1, fold, stream));
    return RDYN_OK;
  }
  int first_col[RDYN_MAX_JOINTS];
  for (int j = 0; j < n; ++j) first_col[j] = 10 * c->active[j];
  double* const ws = (double*)workspace;
  const PanelQrLayout& L = p.L;
  double* const image = ws + L.rows;
  double* const G2 = ws + L.g2;  // Q'Q of [Q | b]: G (cols x cols) | c | bb
  double* const c2 = G2 + (size_t)cols * cols;
  ChunkImage im(c, b, tau_meas, image, cols, &ca, n_comps, K);
  st = im.bind(c->long_chain());
  if (st != RDYN_OK) return st;
  // the chunk images of the ChunkImage writer; k_panel_trmm turns one into Q in place and keeps its zero band zero for the next chunk of
  // the same length, but the right-hand side column is then Q's: without tau_meas (which no writer stores) it has to be zeroed again
  auto write_image = [&](int64_t s0, int64_t cnt, int64_t S) -> int {
    if (cnt == im.cleared_cnt && !tau_meas)
      RDYN_HIP_TRY(hipMemsetAsync(image + (int64_t)cols * n * cnt, 0, sizeof(double) * (size_t)cnt * n, stream));
    return im.write(s0, cnt, S, stream);
  };
  // pass A: one image of every S-th sample (about kPanelQrSubSamples of them, at most one chunk)
  const int64_t sub_cap = p.chunk < kPanelQrSubSamples ? p.chunk : kPanelQrSubSamples;
  const int64_t S = (N + sub_cap - 1) / sub_cap;
  const int64_t sub_cnt = (N + S - 1) / S;
  st = write_image(0, sub_cnt, S);
  if (st != RDYN_OK) return st;
  st = panel_gram_launch(image, (int64_t)n * sub_cnt, (int64_t)n * sub_cnt, cols, image + (int64_t)cols * n * sub_cnt, G2, c2, c2 + cols, 0, true, 0,
                         ws + L.slabs, nullptr, stream, sub_cnt, first_col, n);
  if (st != RDYN_OK) return st;
  double* const R_new = accumulate ? ws + L.r_tmp : R;
  st = panel_qr_rounds(ws, L, n1, tau_meas ? 1 : 0, sqrt((double)N / (double)sub_cnt), R_new, stream, [&](const double* W, const int* run, int) -> int {
    for (int64_t s0 = 0; s0 < N; s0 += p.chunk)
    {
      const int64_t cnt = (N - s0 < p.chunk) ? (N - s0) : p.chunk;
      int s2 = write_image(s0, cnt, 1);
      if (s2 != RDYN_OK) return s2;
      RdynPanelTrmmArgs ta;
      memset(&ta, 0, sizeof ta);
      ta.A = image;
      ta.b = nullptr;
      ta.rows = (int64_t)n * cnt;
      ta.lda = (int64_t)n * cnt;
      ta.n_cols = n1;
      ta.n1 = n1;
      ta.Q = image;
      ta.ldq = (int64_t)n * cnt;
      ta.W = W;
      ta.run_flag = run;
      ta.row_block = cnt;
      for (int j = 0; j < n; ++j) ta.first_col[j] = first_col[j];
      for (int j = n; j < RDYN_MAX_JOINTS; ++j) ta.first_col[j] = 0;
      RDYN_HIP_TRY(rdyn_launch_panel_trmm(ta, stream));
      s2 = panel_gram_launch(image, (int64_t)n * cnt, (int64_t)n * cnt, cols, image + (int64_t)cols * n * cnt, G2, c2, c2 + cols, s0 > 0, s0 + cnt >= N,
                             0, ws + L.slabs, run, stream, cnt, first_col, n);
      if (s2 != RDYN_OK) return s2;
    }
    return RDYN_OK;
  });
  if (st != RDYN_OK) return st;
  if (accumulate) RDYN_HIP_TRY(rdyn_launch_cholqr_fold_global(R_new, R, n1, ws + L.fold, stream));
  return RDYN_OK;
}

size_t rdyn_regressor_tsqr_wide_workspace_bytes(const rdyn_chain* c, int64_t chunk_samples) { return panel_qr_plan(c, nullptr, 0, chunk_samples, false).bytes; }

int rdyn_regressor_tsqr_wide(const rdyn_chain* c, const rdyn_batch* b, const double* tau_meas, double* R, int accumulate, int64_t chunk_samples,
                             void* workspace, size_t workspace_bytes)
{
  return panel_qr_chain_run(c, nullptr, 0, b, tau_meas, R, accumulate, chunk_samples, workspace, workspace_bytes, false);
}

size_t rdyn_identification_tsqr_wide_workspace_bytes(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int64_t chunk_samples)
{
  return panel_qr_plan(c, comps, n_comps, chunk_samples, true).bytes;
}

int rdyn_identification_tsqr_wide(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b, const double* tau_meas,
                                  double* R, int accumulate, int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  return panel_qr_chain_run(c, comps, n_comps, b, tau_meas, R, accumulate, chunk_samples, workspace, workspace_bytes, true);
}
