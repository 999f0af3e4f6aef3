// rdyn_api_gram.cpp -- the normal equations of the C-ABI (include/rdyn.h): rdyn_gram, rdyn_regressor_gram, rdyn_identification_gram and
// the wide variants with their plans; and the chunk-image writer and tile helpers they share with the R factors (rdyn_api_tsqr.cpp).
// The entry points take their C linkage from their declarations in include/rdyn.h.
#include <functional>

#include "rdyn_api_common.h"

// ---- normal equations -----------------------------------------------------------------------------------
static const int kGramBlocks = 512;  // 2 workgroups per CU; each owns one slab of the workspace

static size_t gram_slab_bytes(int n_cols)
{
  const int nb = rdyn_gram_blocks_for(n_cols);
  return (size_t)kGramBlocks * (size_t)(nb * (nb + 1) / 2) * 256 * sizeof(double);
}

size_t rdyn_gram_workspace_bytes(int n_cols) { return (n_cols < 1 || rdyn_gram_blocks_for(n_cols) > 7) ? 0 : gram_slab_bytes(n_cols); }

static int gram_launch(const double* A, int64_t rows, int64_t lda, int n_cols, const double* bvec, double* G, double* cvec, double* bb,
                       int slab_accumulate, bool finish, int add_to_output, void* workspace, hipStream_t st,
                       int64_t row_block = 0, const int* first_col = nullptr, int n_row_blocks = 0)
{
  RdynGramArgs a;
  memset(&a, 0, sizeof a);
  a.row_block = first_col ? row_block : 0;
  for (int j = 0; first_col && j < n_row_blocks && j < RDYN_MAX_SWEPT_JOINTS; ++j) a.first_col[j] = first_col[j];
  a.A = A;
  a.b = bvec;
  a.rows = rows;
  a.lda = lda;
  a.P = n_cols;
  a.accumulate = slab_accumulate;
  a.add_to_output = add_to_output;
  a.slabs = (double*)workspace;
  a.G = G;
  a.c = cvec;
  a.bb = bb;
  RDYN_HIP_TRY(rdyn_launch_gram(a, kGramBlocks, st));
  if (finish) RDYN_HIP_TRY(rdyn_launch_gram_finish(a, kGramBlocks, st));
  return RDYN_OK;
}

int rdyn_gram(const double* A, int64_t rows, int64_t lda, int n_cols, const double* bvec, double* G, double* cvec, double* bb,
              int accumulate, void* workspace, size_t workspace_bytes, int device, void* stream)
{
  if (!A || !G || rows < 0 || lda < rows || n_cols < 1 || !workspace)
  {
    rdyn_set_error("rdyn_gram: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (rdyn_gram_blocks_for(n_cols) > 7)
  {
    rdyn_set_error("rdyn_gram: at most 111 columns are supported");
    return RDYN_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < gram_slab_bytes(n_cols))
  {
    rdyn_set_error("rdyn_gram: workspace too small (%zu < %zu bytes)", workspace_bytes, gram_slab_bytes(n_cols));
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g;
  int st = g.enter(device);
  if (st != RDYN_OK) return st;
  return gram_launch(A, rows, lda, n_cols, bvec, G, cvec, bb, 0, true, accumulate ? 1 : 0, workspace, (hipStream_t)stream);
}

// Fused regressor->Gram kernel: persistent workgroups, each with its own 256-sample tile image (rewritten per tile, so
// it stays in L2 / Infinity Cache): 256 workgroups x 256 samples x n x (P + 1) doubles = 192 MB at n = 6, P = 60.
static const int kFusedBlocks = 256;  // persistent workgroups (one per CU); the workspace is sized for them

// A chain whose own columns exceed what the Gram kernels hold (111) but whose REDUCED companion does not (fixed frames: 10 joints with
// 7 input joints = 100 columns + friction columns) is served through the companion like a chain longer than the kernels sweep.
static bool gram_only_through_reduced(const rdyn_chain* c, int n_comp_cols)
{
  return c->long_chain() || (c->reduced && rdyn_gram_blocks_for(10 * c->n_joints() + n_comp_cols) > 7);
}

// a chain with more input joints than the unrolled kernels sweep (no companion) whose own columns still fit the Gram kernel: 11 input
// joints (110 columns + tau_meas = 111) -- chunk images by rdyn_long_local.hip, contracted by k_gram
static bool gram_by_long_images(const rdyn_chain* c) { return c->long_chain() && !c->reduced && rdyn_gram_blocks_for(10 * c->n_joints()) <= 7; }

size_t rdyn_regressor_gram_workspace_bytes(const rdyn_chain* c, int64_t chunk_samples)
{
  if (!c) return 0;
  if (gram_by_long_images(c))
  {
    const int P = 10 * c->n_joints();
    return align256(gram_slab_bytes(P) + (size_t)default_chunk(chunk_samples) * c->n_active() * (P + 1) * sizeof(double));
  }
  if (gram_only_through_reduced(c, 0))
  {
    // only the reduced companion is swept: its workspace + its normal equations behind it
    const size_t w = c->reduced ? rdyn_regressor_gram_workspace_bytes(c->reduced.get(), 0) : 0;
    return w ? w + reduce_tmp_bytes(10 * c->reduced->n_joints()) : 0;
  }
  const int P = 10 * c->n_joints();
  if (rdyn_gram_blocks_for(P) > 7) return 0;
  const int64_t chunk = default_chunk(chunk_samples);
  const size_t chunked = (size_t)chunk * c->n_active() * (P + 1) * sizeof(double);
  const size_t fused = (size_t)kFusedBlocks * 256 * c->n_active() * (P + 1) * sizeof(double);  // one tile image per workgroup
  const size_t base = align256(gram_slab_bytes(P) + (chunked > fused ? chunked : fused));
  // chains with joints that are not input joints: the kernels run on the reduced companion, whose normal equations wait at the end
  return base + (c->reduced ? reduce_tmp_bytes(10 * c->reduced->n_joints()) : 0);
}

int fill_expand_args(const rdyn_chain* c, int n_red, int K, RdynGramExpandArgs* ea)
{
  memset(ea, 0, sizeof *ea);
  int st = device_expand(c, &ea->X);
  if (st != RDYN_OK) return st;
  for (int f = 0; f < c->n_joints(); ++f) ea->red_of[f] = c->red_of[f];
  ea->n_joints = c->n_joints();
  ea->n_red = n_red;
  ea->n_comp_cols = K;
  return RDYN_OK;
}

// the normal equations of no samples: zeros, or nothing when accumulating
static int zero_normal_equations(double* G, double* cvec, double* bb, int cols, int accumulate, hipStream_t stream)
{
  if (accumulate) return RDYN_OK;
  RDYN_HIP_TRY(hipMemsetAsync(G, 0, sizeof(double) * cols * cols, stream));
  if (cvec) RDYN_HIP_TRY(hipMemsetAsync(cvec, 0, sizeof(double) * cols, stream));
  if (bb) RDYN_HIP_TRY(hipMemsetAsync(bb, 0, sizeof(double), stream));
  return RDYN_OK;
}

// Chains with non-input joints: the normal equations of the reduced companion (rdyn_chain.hpp: every joint an input joint -- the
// fastest instantiations, 10 n instead of 10 nJ columns) into the tail of the workspace, then G = E' G_red E (k_gram_expand).
// companion(G_red, c_red, bb_red, workspace, bytes) is the narrow or the wide call on c->reduced; it gets the workspace in front of the tail.
typedef std::function<int(double* G_red, double* c_red, double* bb_red, void* workspace, size_t workspace_bytes)> CompanionGram;
static int gram_through_reduced(const rdyn_chain* c, int K, const rdyn_batch* b, double* G, double* cvec, double* bb, int accumulate, void* workspace,
                                size_t need_bytes, const CompanionGram& companion)
{
  const rdyn_chain* r = c->reduced.get();
  const int Cr = 10 * r->n_joints() + K;
  const size_t tmp = reduce_tmp_bytes(Cr);
  double* Gr = (double*)((char*)workspace + need_bytes - tmp);
  int st = companion(Gr, Gr + (size_t)Cr * Cr, Gr + (size_t)Cr * Cr + Cr, workspace, need_bytes - tmp);
  if (st != RDYN_OK) return st;
  RdynGramExpandArgs ea;
  st = fill_expand_args(c, r->n_joints(), K, &ea);
  if (st != RDYN_OK) return st;
  ea.G_red = Gr;
  ea.c_red = Gr + (size_t)Cr * Cr;
  ea.bb_red = Gr + (size_t)Cr * Cr + Cr;
  ea.add_to_output = accumulate ? 1 : 0;
  ea.G = G;
  ea.c = cvec;
  ea.bb = bb;
  RDYN_HIP_TRY(rdyn_launch_gram_expand(ea, (hipStream_t)b->stream));
  return RDYN_OK;
}
int ChunkImage::write(int64_t s0, int64_t cnt, int64_t sample_stride, hipStream_t stream)
{
  const int n = c->n_active();
  if (clear && cnt != cleared_cnt)
  {
    RDYN_HIP_TRY(hipMemsetAsync(image, 0, sizeof(double) * (size_t)cnt * n * (cols + 1), stream));
    cleared_cnt = cnt;
  }
  const int64_t in_step = (b->layout == RDYN_LAYOUT_SAMPLE_MAJOR) ? n : 1;  // pointer advance per sample
  const double* const q = b->q + s0 * in_step;
  const double* const dq = b->dq + s0 * in_step;
  const double* const ddq = b->ddq + s0 * in_step;
  const double* const bcol = tau_meas ? tau_meas + s0 * in_step : nullptr;
  int64_t in_ss, in_sj;
  rec_strides(b, n, &in_ss, &in_sj);  // element-major: the joint stride stays the FULL batch's N
  in_ss *= sample_stride;
  if (dl)
  {
    RdynLongLocalArgs a;
    memset(&a, 0, sizeof a);
    a.chain_long = dl;
    a.q = q;
    a.dq = dq;
    a.ddq = ddq;
    a.bcol = bcol;
    a.bcol_col = cols;
    a.n_samples = cnt;
    a.in_ss = in_ss;
    a.in_sj = in_sj;
    a.Y = image;
    a.y_ss = 1;
    a.y_sr = cnt;
    a.y_sc = (int64_t)n * cnt;
    a.n_active = n;
    RDYN_HIP_TRY(rdyn_launch_long_local(RDYN_MODE_REGRESSOR, c->n_joints(), a, stream));
  }
  else
  {
    RdynSweepArgs a;
    memset(&a, 0, sizeof a);
    a.chain = dc;
    a.q = q;
    a.dq = dq;
    a.ddq = ddq;
    a.bcol = bcol;
    a.bcol_col = cols;
    a.n_samples = cnt;
    a.in_ss = in_ss;
    a.in_sj = in_sj;
    a.Y = image;
    a.y_ss = 1;
    a.y_sr = cnt;
    a.y_sc = (int64_t)n * cnt;
    RDYN_HIP_TRY(rdyn_launch_local_sweep(c->n_joints(), RDYN_MODE_REGRESSOR_GRAM, a, stream));
  }
  if (K > 0)
  {
    RdynComponentArgs cc = *ca;
    cc.q = q;
    cc.dq = dq;
    cc.n_samples = cnt;
    cc.in_ss = in_ss;
    cc.in_sj = in_sj;
    cc.n_active = n;
    cc.n_comps = n_comps;
    cc.C = image + (int64_t)10 * c->n_joints() * n * cnt;
    cc.c_ss = 1;
    cc.c_sr = cnt;
    cc.c_sc = (int64_t)n * cnt;
    cc.tau = nullptr;
    RDYN_HIP_TRY(rdyn_launch_components(cc, stream));
  }
  return RDYN_OK;
}

void fill_sw_rows(RdynLdsGramArgs* la, int n, int waves, int slots, int skip)
{
  for (int i = 0; i < 21; ++i) la->sw_rows[i] = 99;
  int load[7] = {0, 0, 0, 0, 0, 0, 0}, used[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int l = 0; l < n && l < 8; ++l)
  {
    int best = -1;
    for (int w = 0; w < waves; ++w)
      if (w != skip && used[w] < slots && (best < 0 || load[w] < load[best])) best = w;
    if (best < 0) return;
    la->sw_rows[3 * best + used[best]++] = l;
    load[best] += n - l;
  }
}
void fill_in_map(const rdyn_chain* c, RdynLdsGramArgs* la)
{
  const int n = c->n_active();
  for (int r = 0; r < 8; ++r) la->in_map[r] = (r < n && r < (int)c->row_input.size()) ? c->row_input[r] : r;
  fill_sw_rows(la, n, 7, 2, n <= 6 ? 3 : -1);
  la->sweep_lanes = 0;
}
int kin_sweeper_pad(const rdyn_chain* c, int n_comp_cols)
{
  if (c->n_active() != c->n_joints()) return 0;
  return rdyn_regressor_gram_duo_kin_pad(c->n_joints(), n_comp_cols);
}
bool build_lds_tile(const rdyn_chain* c, int n_comp_cols, RdynLdsGramArgs* la, bool compact)
{
  // column padding: 4 doubles keep the 16 lanes of an MFMA operand read on disjoint banks; the compact layout (2 doubles, 2-way
  // conflicts on the consumer's reads, which has slack) is what lets four 7-joint tiles WITH component columns fit 160 KB
  const int pad = compact ? 2 : 4;
  const int n = c->n_active(), nJ = c->n_joints();
  bool monotonic = true;
  for (int j = 1; j < n; ++j) monotonic = monotonic && c->active[j] > c->active[j - 1];
  la->all_revolute = 1;
  for (int f = 0; f < nJ; ++f)
    if (c->host_joints[f].type != RDYN_REVOLUTE) la->all_revolute = 0;
  int off = 0;
  for (int f = 0; f < nJ; ++f)
  {
    int m = 0;
    for (int j = 0; j < n; ++j) m += (c->active[j] <= f) ? 1 : 0;
    la->lds_m[f] = m;
    la->lds_stride[f] = (16 * m + pad) * 8;
    la->lds_off[f] = off;
    off += 10 * la->lds_stride[f];
  }
  la->lds_off_c = off;
  la->comp_stride = (16 + pad) * 8;
  off += n_comp_cols * la->comp_stride;
  la->lds_off_b = off;
  off += (16 * n + pad) * 8;
  la->tile_bytes = (int)align256(off);
  la->n_active = n;
  for (int j = 0; j < n; ++j) la->first_col[j] = 10 * c->active[j];
  fill_in_map(c, la);
  return monotonic;
}

int rdyn_regressor_gram(const rdyn_chain* c, const rdyn_batch* b, const double* tau_meas, double* G, double* cvec, double* bb,
                        int accumulate, int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  const bool long_images = c && gram_by_long_images(c);
  int st = check_batch(c, b, true, true, "rdyn_regressor_gram", long_images ? LONG_KERNELS : LONG_COMPANION);
  if (st != RDYN_OK) return st;
  if (!G || !workspace)
  {
    rdyn_set_error("rdyn_regressor_gram: null output or workspace");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  const int n = c->n_active(), P = 10 * c->n_joints();
  // chains with non-input joints: the companion's normal equations (default chunking)
  auto companion = [&](double* Gr, double* cr, double* bbr, void* ws, size_t ws_bytes) {
    return rdyn_regressor_gram(c->reduced.get(), b, tau_meas, Gr, cr, bbr, 0, 0, ws, ws_bytes);
  };
  if (long_images)
  {
    const int64_t chunk = default_chunk(chunk_samples), N = b->n_samples;
    if (workspace_bytes < rdyn_regressor_gram_workspace_bytes(c, chunk))
    {
      rdyn_set_error("rdyn_regressor_gram: workspace too small");
      return RDYN_ERR_INVALID_ARGUMENT;
    }
    DeviceGuard g;
    st = g.enter(b->device);
    if (st != RDYN_OK) return st;
    hipStream_t stream = (hipStream_t)b->stream;
    if (N == 0) return zero_normal_equations(G, cvec, bb, P, accumulate, stream);
    double* const slabs = (double*)workspace;
    ChunkImage im(c, b, tau_meas, (double*)((char*)workspace + gram_slab_bytes(P)), P);
    im.clear = false;  // k_long_regressor stores the structural zeros, and without tau_meas k_gram reads no column P
    st = im.bind(true);
    if (st != RDYN_OK) return st;
    for (int64_t s0 = 0; s0 < N; s0 += chunk)
    {
      const int64_t cnt = (N - s0 < chunk) ? (N - s0) : chunk;
      st = im.write(s0, cnt, 1, stream);
      if (st != RDYN_OK) return st;
      st = gram_launch(im.image, (int64_t)n * cnt, (int64_t)n * cnt, P, tau_meas ? im.image + (int64_t)P * n * cnt : nullptr, G, cvec, bb,
                       s0 > 0 ? 1 : 0, s0 + cnt >= N, accumulate ? 1 : 0, slabs, stream);
      if (st != RDYN_OK) return st;
    }
    return RDYN_OK;
  }
  if (gram_only_through_reduced(c, 0))
  {
    const size_t need = rdyn_regressor_gram_workspace_bytes(c, 0);
    if (need == 0 || workspace_bytes < need)
    {
      rdyn_set_error("rdyn_regressor_gram: %s", need == 0 ? "at most 111 columns of the reduced chain are supported" : "workspace too small");
      return need == 0 ? RDYN_ERR_UNSUPPORTED : RDYN_ERR_INVALID_ARGUMENT;
    }
    DeviceGuard g;
    st = g.enter(b->device);
    if (st != RDYN_OK) return st;
    if (b->n_samples == 0) return zero_normal_equations(G, cvec, bb, P, accumulate, (hipStream_t)b->stream);
    return gram_through_reduced(c, 0, b, G, cvec, bb, accumulate, workspace, need, companion);
  }
  if (rdyn_gram_blocks_for(P) > 7)
  {
    rdyn_set_error("rdyn_regressor_gram: at most 111 regressor columns are supported");
    return RDYN_ERR_UNSUPPORTED;
  }
  const int64_t chunk = default_chunk(chunk_samples);
  if (workspace_bytes < rdyn_regressor_gram_workspace_bytes(c, chunk))
  {
    rdyn_set_error("rdyn_regressor_gram: workspace too small");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  const RdynChainConst* dc = nullptr;
  st = device_const(c, &dc);
  if (st != RDYN_OK) return st;
  hipStream_t stream = (hipStream_t)b->stream;
  double* slabs = (double*)workspace;
  double* scratch = (double*)((char*)workspace + gram_slab_bytes(P));
  const int64_t N = b->n_samples;
  if (N == 0) return zero_normal_equations(G, cvec, bb, P, accumulate, stream);
  // (chunk_samples > 0 keeps the chain as it is: the reference ordering of the two-kernel path)
  if (c->reduced && chunk_samples <= 0)
    return gram_through_reduced(c, 0, b, G, cvec, bb, accumulate, workspace, rdyn_regressor_gram_workspace_bytes(c, chunk), companion);
  // structural zero band of every row block (input joint j): columns < 10 * chain index of joint j
  int first_col[RDYN_MAX_SWEPT_JOINTS];
  for (int j = 0; j < n; ++j) first_col[j] = 10 * c->active[j];
  // RDYN_GRAM_PATH=image (probe builds only, tools/probe_gram_paths.py): the global-image kernel where the wave-pair kernel would run
  const char* path_env = probe_env("RDYN_GRAM_PATH");
  if (chunk_samples <= 0 && n >= 2 && rdyn_regressor_gram_duo_supported(P) && !(path_env && !strcmp(path_env, "image")))
  {
    // wave-pair kernel (rdyn_duo_gram.hip), 2 .. 7 chain joints: needs input joints in chain order (rows of a link's columns are a
    // prefix) and four tiles inside 160 KB of LDS.
    RdynLdsGramArgs la;
    memset(&la, 0, sizeof la);
    // input joints listed out of chain order: the sorted view is swept, every row's inputs read through its map
    const rdyn_chain* const co = ordered(c);
    const int kin_pad = kin_sweeper_pad(co, 0);
    const bool monotonic = build_lds_tile(co, 0, &la, kin_pad == 2);
    const int nb = rdyn_gram_blocks_for(P);
    size_t lds_bytes = 4 * (size_t)la.tile_bytes + (kin_pad ? RDYN_KIN_XCH_BYTES(co->n_joints()) : 0);
    la.sweep_lanes = kin_pad != 0;
    const size_t red_bytes = (size_t)(nb * (nb + 1) / 2) * 256 * sizeof(double);
    if (lds_bytes < red_bytes) lds_bytes = red_bytes;
    if (monotonic && lds_bytes <= 160 * 1024)
    {
      st = device_const(co, &la.chain);
      if (st != RDYN_OK) return st;
      la.q = b->q;
      la.dq = b->dq;
      la.ddq = b->ddq;
      la.bcol = tau_meas;
      la.n_samples = N;
      rec_strides(b, n, &la.in_ss, &la.in_sj);
      la.slabs = slabs;
      const int64_t tiles = (N + 15) / 16;
      const int blocks = (int)((tiles + 3) / 4 < kFusedBlocks ? (tiles + 3) / 4 : kFusedBlocks);
      RDYN_HIP_TRY(rdyn_launch_regressor_gram_duo(P, la, blocks, lds_bytes, stream));
      RdynGramArgs ga;
      memset(&ga, 0, sizeof ga);
      ga.P = P;
      ga.add_to_output = accumulate ? 1 : 0;
      ga.slabs = slabs;
      ga.G = G;
      ga.c = cvec;
      ga.bb = bb;
      ga.desc_nj = c->n_joints();  // the wave-pair kernel accumulates in descending link order
      RDYN_HIP_TRY(rdyn_launch_gram_finish(ga, blocks, stream));
      return RDYN_OK;
    }
  }
  if (chunk_samples <= 0)
  {
    // chains the wave-pair kernel does not take (8 joints: four tiles do not fit the LDS): ONE persistent kernel, the regressor image
    // stays in L2 / Infinity Cache (rdyn_fused_gram.hip).
    // chunk_samples > 0 selects the two-kernel chunked path below (kept for A/B and as the reference ordering).
    RdynFusedGramArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.sweep.chain = dc;
    fa.sweep.q = b->q;
    fa.sweep.dq = b->dq;
    fa.sweep.ddq = b->ddq;
    fa.sweep.bcol = tau_meas;
    fa.sweep.n_samples = N;
    rec_strides(b, n, &fa.sweep.in_ss, &fa.sweep.in_sj);
    fa.n_active = n;
    for (int j = 0; j < n; ++j) fa.first_col[j] = first_col[j];
    fa.images = scratch;
    fa.slabs = slabs;
    const int64_t tiles = (N + 255) / 256;
    const int blocks = (int)(tiles < kFusedBlocks ? tiles : kFusedBlocks);
    // structural zeros that the sweep never stores but the Gram still loads must read as zero
    RDYN_HIP_TRY(hipMemsetAsync(scratch, 0, sizeof(double) * (size_t)blocks * 256 * n * (P + 1), stream));
    RDYN_HIP_TRY(rdyn_launch_regressor_gram_fused(c->n_joints(), fa, blocks, stream));
    RdynGramArgs ga;
    memset(&ga, 0, sizeof ga);
    ga.P = P;
    ga.add_to_output = accumulate ? 1 : 0;
    ga.slabs = slabs;
    ga.G = G;
    ga.c = cvec;  // without tau_meas the image's column P stays zero: c = 0, bb = 0
    ga.bb = bb;
    RDYN_HIP_TRY(rdyn_launch_gram_finish(ga, blocks, stream));
    return RDYN_OK;
  }
  ChunkImage im(c, b, tau_meas, scratch, P);
  im.dc = dc;
  for (int64_t s0 = 0; s0 < N; s0 += chunk)
  {
    const int64_t cnt = (N - s0 < chunk) ? (N - s0) : chunk;
    st = im.write(s0, cnt, 1, stream);
    if (st != RDYN_OK) return st;
    const bool last = (s0 + cnt >= N);
    st = gram_launch(scratch, (int64_t)n * cnt, (int64_t)n * cnt, P, tau_meas ? scratch + (int64_t)P * n * cnt : nullptr, G, cvec, bb,
                     s0 > 0 ? 1 : 0, last, accumulate ? 1 : 0, slabs, stream, cnt, first_col, n);
    if (st != RDYN_OK) return st;
  }
  return RDYN_OK;
}

// ---- identification step: normal equations of [Y | C | tau_meas] (rigid-body regressor + component columns) -------------
static const int64_t kIdentChunk = 131072;  // samples per image chunk (the image of one chunk stays L2 / Infinity-Cache sized)

size_t rdyn_identification_gram_workspace_bytes(const rdyn_chain* c, const rdyn_component* comps, int n_comps)
{
  if (!c) return 0;
  const int K = n_comps > 0 ? rdyn_components_columns(comps, n_comps) : 0;
  if (K >= 0 && gram_only_through_reduced(c, K))
  {
    const size_t w = c->reduced ? rdyn_identification_gram_workspace_bytes(c->reduced.get(), comps, n_comps) : 0;
    return w ? w + reduce_tmp_bytes(10 * c->reduced->n_joints() + K) : 0;
  }
  const int cols = 10 * c->n_joints() + (K > 0 ? K : 0);
  if (K < 0 || rdyn_gram_blocks_for(cols) > 7) return 0;
  const size_t base = align256(gram_slab_bytes(cols) + (size_t)kIdentChunk * c->n_active() * (cols + 1) * sizeof(double));
  return base + (c->reduced ? reduce_tmp_bytes(10 * c->reduced->n_joints() + (K > 0 ? K : 0)) : 0);
}

int rdyn_identification_gram(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b, const double* tau_meas,
                             double* G, double* cvec, double* bb, int accumulate, void* workspace, size_t workspace_bytes)
{
  int st = check_batch(c, b, true, true, "rdyn_identification_gram", LONG_COMPANION);
  if (st != RDYN_OK) return st;
  if (!G || !workspace || n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps))
  {
    rdyn_set_error("rdyn_identification_gram: null output / workspace, or more than %d components", RDYN_MAX_COMPONENTS);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  const int n = c->n_active(), P = 10 * c->n_joints();
  const int K = n_comps > 0 ? rdyn_components_columns(comps, n_comps) : 0;
  const int cols = P + K;
  auto companion = [&](double* Gr, double* cr, double* bbr, void* ws, size_t ws_bytes) {
    const rdyn_chain* r = c->reduced.get();
    return n_comps > 0 ? rdyn_identification_gram(r, comps, n_comps, b, tau_meas, Gr, cr, bbr, 0, ws, ws_bytes)
                       : rdyn_regressor_gram(r, b, tau_meas, Gr, cr, bbr, 0, 0, ws, ws_bytes);
  };
  if (K >= 0 && gram_only_through_reduced(c, K))
  {
    const size_t need = rdyn_identification_gram_workspace_bytes(c, comps, n_comps);
    if (need == 0 || workspace_bytes < need)
    {
      rdyn_set_error("rdyn_identification_gram: %s", need == 0 ? "at most 111 columns (reduced chain + components) are supported" : "workspace too small");
      return need == 0 ? RDYN_ERR_UNSUPPORTED : RDYN_ERR_INVALID_ARGUMENT;
    }
    DeviceGuard g;
    st = g.enter(b->device);
    if (st != RDYN_OK) return st;
    if (b->n_samples == 0) return zero_normal_equations(G, cvec, bb, cols, accumulate, (hipStream_t)b->stream);
    return gram_through_reduced(c, K, b, G, cvec, bb, accumulate, workspace, need, companion);
  }
  if (rdyn_gram_blocks_for(cols) > 7)
  {
    rdyn_set_error("rdyn_identification_gram: at most 111 columns (regressor + components) are supported");
    return RDYN_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < rdyn_identification_gram_workspace_bytes(c, comps, n_comps))
  {
    rdyn_set_error("rdyn_identification_gram: workspace too small");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  RdynComponentArgs ca;
  memset(&ca, 0, sizeof ca);
  st = fill_components(comps, n_comps, n, &ca);
  if (st != RDYN_OK) return st;
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  const RdynChainConst* dc = nullptr;
  st = device_const(c, &dc);
  if (st != RDYN_OK) return st;
  hipStream_t stream = (hipStream_t)b->stream;
  double* slabs = (double*)workspace;
  double* scratch = (double*)((char*)workspace + gram_slab_bytes(cols));
  const int64_t N = b->n_samples;
  if (N == 0) return zero_normal_equations(G, cvec, bb, cols, accumulate, stream);
  if (c->reduced)
    return gram_through_reduced(c, K, b, G, cvec, bb, accumulate, workspace, rdyn_identification_gram_workspace_bytes(c, comps, n_comps), companion);
  // ---- fused: regressor rows AND component columns stay in LDS (rdyn_duo_gram.hip); else the chunk image below
  if (n >= 2 && n <= 8 && rdyn_regressor_gram_duo_supports_components(P, K))
  {
    RdynLdsGramArgs la;
    memset(&la, 0, sizeof la);
    const rdyn_chain* const co = ordered(c);  // (input joints out of chain order: the sorted view, rdyn_chain.hpp)
    bool monotonic = build_lds_tile(co, K, &la);
    if (4 * (size_t)la.tile_bytes > 160 * 1024) monotonic = build_lds_tile(co, K, &la, true);  // compact layout (7 joints + components)
    const int nbt = K > 0 ? rdyn_gram_blocks_for(P) + 1 : rdyn_gram_blocks_for(P);  // the kernel's slab layout (XB = 1 with components)
    size_t lds_bytes = 4 * (size_t)la.tile_bytes;
    if (kin_sweeper_pad(co, K) == 4 && lds_bytes + RDYN_KIN_XCH_BYTES(co->n_joints()) <= 160 * 1024 && la.lds_stride[0] == (16 + 4) * 8)
    {
      la.sweep_lanes = 1;  // one lane per sample: the exchange area behind the tiles
      lds_bytes += RDYN_KIN_XCH_BYTES(co->n_joints());
    }
    const size_t red_bytes = (size_t)(nbt * (nbt + 1) / 2) * 256 * sizeof(double);
    if (lds_bytes < red_bytes) lds_bytes = red_bytes;
    if (monotonic && lds_bytes <= 160 * 1024)
    {
      st = device_const(co, &la.chain);
      if (st != RDYN_OK) return st;
      la.q = b->q;
      la.dq = b->dq;
      la.ddq = b->ddq;
      la.bcol = tau_meas;
      la.n_samples = N;
      rec_strides(b, n, &la.in_ss, &la.in_sj);
      la.slabs = slabs;
      la.n_comps = n_comps;
      la.n_comp_cols = K;
      int col = 0;
      for (int i = 0; i < n_comps; ++i)
      {
        la.comps[i] = ca.comps[i];
        la.comps[i].joint = co->input_row[ca.comps[i].joint];  // the tile row of the component's input joint
        const int w = ca.comps[i].type == RDYN_COMP_FRICTION2 ? 3 : 2;
        for (int k = 0; k < w; ++k) la.comp_col_row[col++] = (signed char)la.comps[i].joint;
      }
      const int64_t tiles = (N + 15) / 16;
      const int blocks = (int)((tiles + 3) / 4 < kFusedBlocks ? (tiles + 3) / 4 : kFusedBlocks);
      RDYN_HIP_TRY(rdyn_launch_regressor_gram_duo(P, la, blocks, lds_bytes, stream));
      RdynGramArgs ga;
      memset(&ga, 0, sizeof ga);
      ga.desc_nj = c->n_joints();  // the kernel accumulates in the order [component columns | tau_meas | links descending]
      ga.desc_k = K;
      ga.slab_nb = nbt;
      ga.P = cols;
      ga.add_to_output = accumulate ? 1 : 0;
      ga.slabs = slabs;
      ga.G = G;
      ga.c = cvec;
      ga.bb = bb;
      RDYN_HIP_TRY(rdyn_launch_gram_finish(ga, blocks, stream));
      return RDYN_OK;
    }
  }
  int first_col[RDYN_MAX_SWEPT_JOINTS];
  for (int j = 0; j < n; ++j) first_col[j] = 10 * c->active[j];  // the component columns lie to the right: always loaded
  ChunkImage im(c, b, tau_meas, scratch, cols, &ca, n_comps, K);
  im.dc = dc;
  for (int64_t s0 = 0; s0 < N; s0 += kIdentChunk)
  {
    const int64_t cnt = (N - s0 < kIdentChunk) ? (N - s0) : kIdentChunk;
    st = im.write(s0, cnt, 1, stream);
    if (st != RDYN_OK) return st;
    const bool last = (s0 + cnt >= N);
    st = gram_launch(scratch, (int64_t)n * cnt, (int64_t)n * cnt, cols, tau_meas ? scratch + (int64_t)cols * n * cnt : nullptr, G, cvec, bb,
                     s0 > 0 ? 1 : 0, last, accumulate ? 1 : 0, slabs, stream, cnt, first_col, n);
    if (st != RDYN_OK) return st;
  }
  return RDYN_OK;
}

// ---- normal equations wider than 111 columns: the column-panel Gram (rdyn_panel_gram.hip) -----------------------------------------
// Default chunk: as many samples as keep one chunk image [Y | C | tau_meas] within 128 MiB (inside the 256 MiB Infinity Cache), but
// never fewer than kWideMinChunk.  Measured (profiles/r7/wide_gram.txt): the image writers cost a fixed ~0.36 ms per launch at 32
// input joints up to 16 384 samples, so the cache-sized chunk of 1 600 samples took 35.5 ms per 1e5 samples against 14.5 ms at 16 384;
// the panel pairs' re-reads run at the same rate whether the matrix fits the Infinity Cache or not.
static const int64_t kWideImageBytes = (int64_t)128 << 20;
static const int64_t kWideMinChunk = 16384;

int64_t wide_chunk(const rdyn_chain* c, int cols, int64_t chunk_samples)
{
  const int64_t fit = (kWideImageBytes / ((int64_t)c->n_active() * (cols + 1) * (int64_t)sizeof(double))) & ~(int64_t)63;
  return chunk_samples > 0 ? chunk_samples : (fit > kWideMinChunk ? fit : kWideMinChunk);
}

size_t rdyn_gram_wide_workspace_bytes(int n_cols)
{
  return (n_cols < 1 || n_cols > RDYN_MAX_WIDE_COLUMNS) ? 0 : panel_slab_bytes(n_cols);
}

int panel_gram_launch(const double* A, int64_t rows, int64_t lda, int n_cols, const double* bvec, double* G, double* cvec, double* bb,
                      int slab_accumulate, bool finish, int add_to_output, void* slabs, const int* run_flag, hipStream_t st, int64_t row_block,
                      const int* first_col, int n_row_blocks)
{
  RdynPanelGramArgs a;
  memset(&a, 0, sizeof a);
  a.row_block = first_col ? row_block : 0;
  for (int j = 0; first_col && j < n_row_blocks && j < RDYN_MAX_JOINTS; ++j) a.first_col[j] = first_col[j];
  a.A = A;
  a.b = bvec;
  a.rows = rows;
  a.lda = lda;
  a.P = n_cols;
  a.accumulate = slab_accumulate;
  a.add_to_output = add_to_output;
  a.slabs = (double*)slabs;
  a.G = G;
  a.c = cvec;
  a.bb = bb;
  a.run_flag = run_flag;
  RDYN_HIP_TRY(rdyn_launch_panel_gram(a, st));
  if (finish) RDYN_HIP_TRY(rdyn_launch_panel_gram_finish(a, st));
  return RDYN_OK;
}

int rdyn_gram_wide(const double* A, int64_t rows, int64_t lda, int n_cols, const double* bvec, double* G, double* cvec, double* bb,
                   int accumulate, void* workspace, size_t workspace_bytes, int device, void* stream)
{
  if (!A || !G || rows < 0 || lda < rows || n_cols < 1 || !workspace)
  {
    rdyn_set_error("rdyn_gram_wide: invalid argument");
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (n_cols > RDYN_MAX_WIDE_COLUMNS)
  {
    rdyn_set_error("rdyn_gram_wide: at most %d columns are supported", RDYN_MAX_WIDE_COLUMNS);
    return RDYN_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < panel_slab_bytes(n_cols))
  {
    rdyn_set_error("rdyn_gram_wide: workspace too small (%zu < %zu bytes)", workspace_bytes, panel_slab_bytes(n_cols));
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g;
  int st = g.enter(device);
  if (st != RDYN_OK) return st;
  return panel_gram_launch(A, rows, lda, n_cols, bvec, G, cvec, bb, 0, true, accumulate ? 1 : 0, workspace, nullptr, (hipStream_t)stream);
}

// How a wide request is served: by the narrow call (it already serves it), through the reduced companion (the wide normal equations
// of the companion, then k_gram_expand), or by chunk images of the chain itself (more than RDYN_MAX_SWEPT_JOINTS input joints:
// k_long_regressor; a swept chain: the element-major regressor sweep) with the component columns behind Y, into the panel kernel.
enum { WIDE_NONE = 0, WIDE_NARROW, WIDE_REDUCED, WIDE_LONG_IMAGES, WIDE_SWEEP_IMAGES };
struct WidePlan
{
  int route = WIDE_NONE;
  int K = 0, cols = 0;
  int64_t chunk = 0;
  size_t bytes = 0;  // workspace
};

static WidePlan wide_plan(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int64_t chunk_samples, bool ident)
{
  WidePlan p;
  if (!c || c->n_joints() < 1 || n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps)) return p;
  p.K = n_comps > 0 ? rdyn_components_columns(comps, n_comps) : 0;
  p.cols = 10 * c->n_joints() + p.K;
  const size_t narrow = ident ? rdyn_identification_gram_workspace_bytes(c, comps, n_comps) : rdyn_regressor_gram_workspace_bytes(c, chunk_samples);
  if (narrow > 0)
  {
    p.route = WIDE_NARROW;
    p.bytes = narrow;
    return p;
  }
  if (p.cols > RDYN_MAX_WIDE_COLUMNS) return p;
  if (c->reduced)
  {
    const WidePlan r = wide_plan(c->reduced.get(), comps, n_comps, chunk_samples, ident);
    if (r.bytes == 0) return p;
    p.route = WIDE_REDUCED;
    p.bytes = r.bytes + reduce_tmp_bytes(10 * c->reduced->n_joints() + p.K);
    return p;
  }
  p.route = c->long_chain() ? WIDE_LONG_IMAGES : WIDE_SWEEP_IMAGES;
  p.chunk = wide_chunk(c, p.cols, chunk_samples);
  p.bytes = panel_slab_bytes(p.cols) + align256((size_t)p.chunk * c->n_active() * (p.cols + 1) * sizeof(double));
  return p;
}

static int gram_wide_run(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b, const double* tau_meas, double* G,
                         double* cvec, double* bb, int accumulate, int64_t chunk_samples, void* workspace, size_t workspace_bytes, bool ident)
{
  const char* fn = ident ? "rdyn_identification_gram_wide" : "rdyn_regressor_gram_wide";
  int st = check_batch(c, b, true, true, fn, LONG_KERNELS);
  if (st != RDYN_OK) return st;
  if (!G || !workspace || n_comps < 0 || n_comps > RDYN_MAX_COMPONENTS || (n_comps > 0 && !comps))
  {
    rdyn_set_error("%s: null output / workspace, or more than %d components", fn, RDYN_MAX_COMPONENTS);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  const int n = c->n_active();
  RdynComponentArgs ca;
  memset(&ca, 0, sizeof ca);
  st = fill_components(comps, n_comps, n, &ca);
  if (st != RDYN_OK) return st;
  const WidePlan p = wide_plan(c, comps, n_comps, chunk_samples, ident);
  if (p.bytes == 0)
  {
    rdyn_set_error("%s: at most %d columns (regressor + components) are supported", fn, RDYN_MAX_WIDE_COLUMNS);
    return RDYN_ERR_UNSUPPORTED;
  }
  if (workspace_bytes < p.bytes)
  {
    rdyn_set_error("%s: workspace too small (%zu < %zu bytes)", fn, workspace_bytes, p.bytes);
    return RDYN_ERR_INVALID_ARGUMENT;
  }
  if (p.route == WIDE_NARROW)
    return ident ? rdyn_identification_gram(c, comps, n_comps, b, tau_meas, G, cvec, bb, accumulate, workspace, workspace_bytes)
                 : rdyn_regressor_gram(c, b, tau_meas, G, cvec, bb, accumulate, chunk_samples, workspace, workspace_bytes);
  DeviceGuard g;
  st = g.enter(b->device);
  if (st != RDYN_OK) return st;
  hipStream_t stream = (hipStream_t)b->stream;
  const int cols = p.cols, K = p.K;
  const int64_t N = b->n_samples;
  if (N == 0) return zero_normal_equations(G, cvec, bb, cols, accumulate, stream);
  if (p.route == WIDE_REDUCED)
    return gram_through_reduced(c, K, b, G, cvec, bb, accumulate, workspace, p.bytes,
                                [&](double* Gr, double* cr, double* bbr, void* ws, size_t ws_bytes) {
                                  return gram_wide_run(c->reduced.get(), comps, n_comps, b, tau_meas, Gr, cr, bbr, 0, chunk_samples, ws, ws_bytes, ident);
                                });
  // chunk images (ChunkImage); row block j is zero left of column 10 * (chain index of input joint j) -- the component columns lie to
  // the right of every band
  ChunkImage im(c, b, tau_meas, (double*)((char*)workspace + panel_slab_bytes(cols)), cols, &ca, n_comps, K);
  st = im.bind(p.route == WIDE_LONG_IMAGES);
  if (st != RDYN_OK) return st;
  int first_col[RDYN_MAX_JOINTS];
  for (int j = 0; j < n; ++j) first_col[j] = 10 * c->active[j];
  double* const slabs = (double*)workspace;
  for (int64_t s0 = 0; s0 < N; s0 += p.chunk)
  {
    const int64_t cnt = (N - s0 < p.chunk) ? (N - s0) : p.chunk;
    st = im.write(s0, cnt, 1, stream);
    if (st != RDYN_OK) return st;
    st = panel_gram_launch(im.image, (int64_t)n * cnt, (int64_t)n * cnt, cols, tau_meas ? im.image + (int64_t)cols * n * cnt : nullptr, G, cvec, bb,
                           s0 > 0 ? 1 : 0, s0 + cnt >= N, accumulate ? 1 : 0, slabs, nullptr, stream, cnt, first_col, n);
    if (st != RDYN_OK) return st;
  }
  return RDYN_OK;
}

size_t rdyn_regressor_gram_wide_workspace_bytes(const rdyn_chain* c, int64_t chunk_samples) { return wide_plan(c, nullptr, 0, chunk_samples, false).bytes; }

int rdyn_regressor_gram_wide(const rdyn_chain* c, const rdyn_batch* b, const double* tau_meas, double* G, double* cvec, double* bb,
                             int accumulate, int64_t chunk_samples, void* workspace, size_t workspace_bytes)
{
  return gram_wide_run(c, nullptr, 0, b, tau_meas, G, cvec, bb, accumulate, chunk_samples, workspace, workspace_bytes, false);
}

size_t rdyn_identification_gram_wide_workspace_bytes(const rdyn_chain* c, const rdyn_component* comps, int n_comps, int64_t chunk_samples)
{
  return wide_plan(c, comps, n_comps, chunk_samples, true).bytes;
}

int rdyn_identification_gram_wide(const rdyn_chain* c, const rdyn_component* comps, int n_comps, const rdyn_batch* b, const double* tau_meas,
                                  double* G, double* cvec, double* bb, int accumulate, int64_t chunk_samples, void* workspace,
                                  size_t workspace_bytes)
{
  return gram_wide_run(c, comps, n_comps, b, tau_meas, G, cvec, bb, accumulate, chunk_samples, workspace, workspace_bytes, true);
}
