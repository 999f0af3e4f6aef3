// rdyn_panel_trmm.hip -- pass B of the column-panel CholeskyQR (rdyn_tsqr_wide): Q = X W on the fp64 matrix cores (gfx950).
//
// X is [A | b] (rows x n1, column-major), W = T^-1 the upper-triangular n1 x n1 preconditioner of k_cholqr_precond<.., PANEL>, stored in
// its MFMA operand order (per block pair cb1 <= cb2 four k-steps of 64 doubles: W[16 cb1 + 4 kk + g][16 cb2 + c] at lane c + 16 g).  The
// product is the Gram input of the round: k_panel_gram reduces Q'Q afterwards.  W of 416 columns is 0.7 MB and does not fit the LDS;
// it is read from L2 (every workgroup walks the same W, the rows of X differ).
//
// One workgroup per 64 rows, one wave per column panel of four 16-column blocks (ceil(n1 / 64) waves).  Wave J accumulates the 4 x 4
// tiles (16 rows x 16 columns) of its panel: output block cb = 4 J + cl sums X(:, kb) W(kb, cb) over kb <= cb.  The operands are
// swapped against k_pgram_rows (A = W^T, B = X^T: the product comes out TRANSPOSED), so that a result register holds 16 consecutive
// rows of one column -- the stores are 128-byte column segments, as the panel Gram reads them.  Each X operand feeds four MFMAs, each
// W operand four.  W(kb, cb) for kb > cb (the diagonal panel's tail) and columns beyond n1 enter as zeros.
//
// rdyn_tsqr_wide: Q is a row chunk of the workspace (the caller's A is const), the rows walked chunk by chunk, each chunk's Q'Q summed
// into the panel Gram's slabs.  The chain forms: in place (Q == A, the chunk image; nothing wider than one chunk is stored) -- every wave
// of the workgroup reads its 64 rows into its accumulators before the barrier and only then writes them; workgroups own disjoint rows.
//
// Zero band of a chunk image (row_block > 0): row block j is zero left of column first_col[j]; the upper-triangular W keeps it zero in
// Q.  The column blocks wholly inside the band of every row of the workgroup are skipped (loads and MFMAs); their output is the exact
// zero the product gives.  fp64 throughout, no atomics, every sum in a fixed order: bitwise reproducible.
#include <hip/hip_runtime.h>
#include "rdyn_kernels.h"
#include "rdyn_gram_common.h"

namespace
{
constexpr int kRows = 64;       // rows per workgroup: four 16-row tiles per wave
constexpr int kMaxPanels = 7;   // ceil(416 / 64)

__global__ __launch_bounds__(64 * kMaxPanels) void k_panel_trmm(const RdynPanelTrmmArgs a)
{
  if (a.run_flag && *a.run_flag == 0) return;
  const int lane = threadIdx.x & 63;
  const int J = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int n1 = a.n1, NB = (n1 + 15) >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * kRows;

  // first column block that is not zero in every row of this workgroup (the minimum over the row blocks its rows touch)
  int kb0 = 0;
  if (a.row_block > 0)
  {
    const int64_t last = (r0 + kRows <= a.rows ? r0 + kRows : a.rows) - 1;
    const int jl = (int)(last / a.row_block);
    int fc = 1 << 30;
    for (int j = (int)(r0 / a.row_block); j <= jl && j < RDYN_MAX_JOINTS; ++j) fc = a.first_col[j] < fc ? a.first_col[j] : fc;
    kb0 = fc >> 4;
  }

  d4 acc[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int cl = 0; cl < 4; ++cl) acc[rt][cl] = (d4){0.0, 0.0, 0.0, 0.0};

  const int kb_end = (4 * J + 4 < NB ? 4 * J + 4 : NB);  // one past the last block with W(kb, cb) != 0 for a cb of this panel
  for (int kb = kb0; kb < kb_end; ++kb)
  {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
    {
      const int p = 16 * kb + 4 * kk + g;  // this lane's column of X
      const double* col = p < a.n_cols ? a.A + (int64_t)p * a.lda : ((p == a.n_cols && p < n1) ? a.b : nullptr);
      double x[4], w[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
      {
        const int64_t r = r0 + 16 * rt + c;
        x[rt] = (col && r < a.rows) ? col[r] : 0.0;
      }
#pragma unroll
      for (int cl = 0; cl < 4; ++cl)
      {
        const int cb = 4 * J + cl;
        w[cl] = (kb <= cb && cb < NB) ? a.W[((int64_t)(cb * (cb + 1) / 2 + kb) * 4 + kk) * 64 + lane] : 0.0;
      }
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int cl = 0; cl < 4; ++cl) acc[rt][cl] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[cl], x[rt], acc[rt][cl], 0, 0, 0);
    }
  }

  __syncthreads();  // in place: every wave has read the workgroup's rows
  // result register t of lane (c, g): Q(row 16 rt + c, column 16 cb + g + 4 t)
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
  {
    const int64_t r = r0 + 16 * rt + c;
    if (r >= a.rows) continue;
#pragma unroll
    for (int cl = 0; cl < 4; ++cl)
#pragma unroll
      for (int t = 0; t < 4; ++t)
      {
        const int col = 16 * (4 * J + cl) + g + 4 * t;
        if (col < n1) a.Q[(int64_t)col * a.ldq + r] = acc[rt][cl][t];
      }
  }
}
// the preconditioner's row subsample of a materialised matrix: 16-row group v of Q = group v * gs of [A | b] (one thread per element)
__global__ __launch_bounds__(256) void k_panel_gather(const double* __restrict__ A, const double* __restrict__ b, int64_t rows, int64_t lda, int n_cols,
                                                      int64_t gs, double* __restrict__ Q, int64_t ldq, int64_t q_rows)
{
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int col = blockIdx.y;
  if (i >= q_rows) return;
  const int64_t r = (i >> 4) * gs * 16 + (i & 15);
  const double* src = col < n_cols ? A + (int64_t)col * lda : b;
  Q[(int64_t)col * ldq + i] = r < rows ? src[r] : 0.0;
}
}  // namespace

int64_t rdyn_panel_gather_rows(int64_t rows, int64_t group_stride)
{
  const int64_t groups = (rows + 15) / 16;
  return ((groups + group_stride - 1) / group_stride) * 16;
}

hipError_t rdyn_launch_panel_gather(const double* A, const double* b, int64_t rows, int64_t lda, int n_cols, int64_t group_stride, double* Q,
                                    int64_t ldq, hipStream_t st)
{
  const int64_t q_rows = rdyn_panel_gather_rows(rows, group_stride);
  if (group_stride < 1 || ldq < q_rows || n_cols < 1) return hipErrorInvalidValue;
  if (q_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(k_panel_gather, dim3((unsigned)((q_rows + 255) / 256), (unsigned)(n_cols + (b ? 1 : 0))), dim3(256), 0, st, A, b, rows, lda,
                     n_cols, group_stride, Q, ldq, q_rows);
  return hipGetLastError();
}

hipError_t rdyn_launch_panel_trmm(const RdynPanelTrmmArgs& a, hipStream_t st)
{
  if (a.n1 < 1 || a.n1 > 16 * 4 * kMaxPanels || a.rows < 0 || a.ldq < a.rows || !a.Q || !a.W) return hipErrorInvalidValue;
  if (a.rows == 0) return hipSuccess;
  const int panels = ((a.n1 + 15) / 16 + 3) / 4;
  hipLaunchKernelGGL(k_panel_trmm, dim3((unsigned)((a.rows + kRows - 1) / kRows)), dim3(64 * panels), 0, st, a);
  return hipGetLastError();
}
