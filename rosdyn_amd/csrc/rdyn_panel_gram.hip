// rdyn_panel_gram.hip -- normal equations wider than k_gram holds: a column-panel Gram on the fp64 matrix cores (gfx950).
//
// k_gram (rdyn_gram.hip) keeps every upper tile of [A | b] in registers, which stops at seven 16-column blocks (111 columns + b).
// Here the NB = ceil((P + 1) / 16) column blocks of [A | b] are cut into panels of PB blocks, and ONE launch covers every panel
// pair (I <= J): blockIdx.y = pair index (J outer, I <= J inner), blockIdx.x = row-slice workgroup.  A diagonal pair holds the
// PB (PB + 1) / 2 upper tiles of its panel, an off-diagonal pair all PB^2 tiles of panel I x panel J; every pair re-reads the rows
// of its two panels.  All workgroups walk their rows with the same stride, so the pairs read the same rows at about the same time
// (the re-reads of the chunk images come from the Infinity Cache).
//
// Operand feed, MFMA and determinism are k_gram's: lane (c, g) loads four consecutive rows (32 B) of column 16 cb + c,
// v_mfma_f64_16x16x4_f64, the waves summed through LDS in wave order, one slab per workgroup (no atomics), k_panel_gram_finish sums
// the slabs in fixed order and scatters G (both triangles), c = A^T b and bb = b^T b.
//
// Zero band of the regressor images (row_block > 0): the rows of input joint j are zero in the columns < first_col[j].  A 16-row group
// whose band covers all of panel I adds nothing to pair (I, J): it is skipped whole, loads included (a wave jumps over the rest of a
// row block at once).  Inside a group the column blocks of panel I left of the band are skipped with one wave-uniform switch between
// straight-line MFMA blocks (as k_gram<NB, true>; the matrix without bands takes an instantiation without the switch, see the note in
// rdyn_gram.hip on accumulators copied where branches meet).
#include <hip/hip_runtime.h>
#include "rdyn_kernels.h"
#include "rdyn_gram_common.h"

namespace
{
constexpr int PB = RDYN_PANEL_BLOCKS;  // 16-column blocks per panel
constexpr int SLAB = PB * PB * 256;    // doubles per workgroup slab (a diagonal pair uses the first PB (PB + 1) / 2 tiles)

// the 4 k-steps of one 16-row group for the PB x PB tiles of an off-diagonal pair, tile t = cb * PB + rb, rows rb >= S of panel I
template <int S>
__device__ __forceinline__ void mfma_pair(const d4* ci, const d4* cj, d4* acc)
{
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int cb = 0; cb < PB; ++cb)
#pragma unroll
      for (int rb = S; rb < PB; ++rb)
        acc[cb * PB + rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ci[rb][t], cj[cb][t], acc[cb * PB + rb], 0, 0, 0);
}

template <bool DIAG, int S>
__device__ __forceinline__ void mfma_block(const d4* cur, d4* acc)
{
  if constexpr (DIAG)
    mfma_group<PB, S>(cur, acc);  // upper tiles t = cb (cb + 1) / 2 + rb
  else
    mfma_pair<S>(cur, cur + PB, acc);
}

#define RDYN_PANEL_CASE(S) \
  case S:                  \
    if constexpr (S < PB) mfma_block<DIAG, S>(cur, acc); \
    break;

template <bool DIAG, bool BANDS>
__device__ __forceinline__ void panel_pair(const RdynPanelGramArgs& a, int I, int J, int pair, double* red)
{
  constexpr int NT = DIAG ? PB * (PB + 1) / 2 : PB * PB;
  constexpr int NL = DIAG ? PB : 2 * PB;  // operand blocks per 16-row group: panel I (and panel J)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int64_t R = a.rows;

  // per-lane column base pointers (null -> column of zeros: padding beyond P + 1)
  const double* col[NL];
#pragma unroll
  for (int k = 0; k < NL; ++k)
  {
    const int p = 16 * (k < PB ? PB * I + k : PB * J + k - PB) + c;
    col[k] = (p < a.P) ? a.A + (int64_t)p * a.lda : ((p == a.P && a.b) ? a.b : nullptr);
  }

  d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};

  const int64_t wstride = (int64_t)gridDim.x * 4 * 16;
  int jb = 0;
  int64_t bound = a.row_block;  // rows < bound belong to row block jb (rows only grow: tracked incrementally)
  // column blocks of panel I that are zero in the 16-row group at r (wave-uniform); PB = the whole group adds nothing
  auto skip_of = [&](int64_t r) -> int {
    if (!BANDS) return 0;
    while (r >= bound && jb + 1 < RDYN_MAX_JOINTS)
    {
      ++jb;
      bound += a.row_block;
    }
    // a group may straddle row blocks (short chunks) and first_col is not monotonic: the minimum over every block it touches
    int fc = a.first_col[jb];
    int j2 = jb + 1;
    for (int64_t b2 = bound; b2 <= r + 15 && b2 < R && j2 < RDYN_MAX_JOINTS; b2 += a.row_block, ++j2)
      if (a.first_col[j2] < fc) fc = a.first_col[j2];
    const int s = (fc >> 4) - PB * I;
    return s < 0 ? 0 : (s > PB ? PB : s);
  };
  // this wave's first 16-row group at or after r that adds something to the pair
  auto next_group = [&](int64_t r, int& s) -> int64_t {
    while (r < R)
    {
      s = skip_of(r);
      if (s < PB) return r;
      // the rest of row block jb adds nothing either: go on with the first group that reaches into the next block
      const int64_t k = (bound - 15 - r + wstride - 1) / wstride;
      r += (k > 1 ? k : 1) * wstride;
    }
    return r;
  };

  auto load = [&](int64_t rbase, int s, d4* v) {
    const int64_t r = rbase + 4 * g;
#pragma unroll
    for (int k = 0; k < NL; ++k)
    {
      d4 x = (d4){0.0, 0.0, 0.0, 0.0};
      if ((k >= PB || k >= s) && col[k])
      {
        if (r + 4 <= R)
          x = *(const d4u*)(col[k] + r);
        else
        {
          if (r + 0 < R) x[0] = col[k][r + 0];
          if (r + 1 < R) x[1] = col[k][r + 1];
          if (r + 2 < R) x[2] = col[k][r + 2];
        }
      }
      v[k] = x;
    }
  };

  d4 cur[NL], nxt[NL];
  int s = 0, s_n = 0;
  int64_t r0 = next_group(((int64_t)blockIdx.x * 4 + wave) * 16, s);
  if (r0 < R) load(r0, s, cur);
  while (r0 < R)
  {
    const int64_t rn = next_group(r0 + wstride, s_n);
    if (rn < R) load(rn, s_n, nxt);  // prefetch the next group behind this group's MFMAs
    if constexpr (BANDS)
    {
      switch (s)
      {
        RDYN_PANEL_CASE(0)
        RDYN_PANEL_CASE(1)
        RDYN_PANEL_CASE(2)
        RDYN_PANEL_CASE(3)
        RDYN_PANEL_CASE(4)
        RDYN_PANEL_CASE(5)
        RDYN_PANEL_CASE(6)
        RDYN_PANEL_CASE(7)
      default: break;
      }
    }
    else
      mfma_block<DIAG, 0>(cur, acc);
#pragma unroll
    for (int k = 0; k < NL; ++k) cur[k] = nxt[k];
    s = s_n;
    r0 = rn;
  }

  gram_block_reduce_to_slab<NT>(acc, red, wave, c, g, a.slabs + ((int64_t)pair * gridDim.x + blockIdx.x) * SLAB, a.accumulate != 0);
}
#undef RDYN_PANEL_CASE

__device__ __forceinline__ void pair_of(int pair, int& I, int& J)
{
  J = 0;
  while ((J + 1) * (J + 2) / 2 <= pair) ++J;
  I = pair - J * (J + 1) / 2;
}

// GATED: the pass of a CholeskyQR round that may not be needed (rdyn_tsqr_wide): leaves at once when *run_flag == 0
template <bool BANDS, bool GATED = false>
__global__ __launch_bounds__(256) void k_panel_gram(const RdynPanelGramArgs a)
{
  if (GATED && *a.run_flag == 0) return;
  __shared__ double red[PB * PB * 256];
  const int pair = blockIdx.y;
  int I, J;
  pair_of(pair, I, J);
  if (I == J)
    panel_pair<true, BANDS>(a, I, J, pair, red);
  else
    panel_pair<false, BANDS>(a, I, J, pair, red);
}

// sums the slabs of every pair (fixed order) and scatters the tiles into G (P x P, both triangles), c, bb: one workgroup per 32 slab
// elements, FG groups of 32 threads split the row-slice workgroups, the groups summed through LDS in fixed order (as k_gram_finish)
constexpr int FG = 32;
template <bool GATED = false>
__global__ __launch_bounds__(32 * FG) void k_panel_gram_finish(const RdynPanelGramArgs a, int pairs, int gx)
{
  if (GATED && *a.run_flag == 0) return;
  const int e_loc = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int64_t i = (int64_t)blockIdx.x * 32 + e_loc;
  const int pair = (int)(i / SLAB), loc = (int)(i % SLAB);
  const int t = loc >> 8, e = loc & 255;
  int I = 0, J = 0;
  if (pair < pairs) pair_of(pair, I, J);
  const bool live = pair < pairs && (I != J || t < PB * (PB + 1) / 2);
  __shared__ double part[FG][32];
  double s = 0.0;
  if (live)
    for (int b = grp; b < gx; b += FG) s += a.slabs[((int64_t)pair * gx + b) * SLAB + loc];
  part[grp][e_loc] = s;
  __syncthreads();
  if (grp != 0 || !live) return;
  s = 0.0;
  for (int k = 0; k < FG; ++k) s += part[k][e_loc];
  int rb, cb;
  if (I == J)
  {
    cb = 0;
    while ((cb + 1) * (cb + 2) / 2 <= t) ++cb;
    rb = t - cb * (cb + 1) / 2;
  }
  else
  {
    cb = t / PB;
    rb = t - cb * PB;
  }
  rb += PB * I;
  cb += PB * J;
  const int p1 = 16 * rb + (e >> 4), p2 = 16 * cb + (e & 15);
  const int P = a.P;
  // overwrite (whatever the outputs held, NaN included) or add
  auto put = [&](double* y) { *y = a.add_to_output ? *y + s : s; };
  if (rb == cb && p1 > p2) return;  // diagonal tiles hold both triangles: keep the upper one
  if (p1 < P && p2 < P)
  {
    put(a.G + (int64_t)p2 * P + p1);
    if (p1 != p2) put(a.G + (int64_t)p1 * P + p2);
  }
  else if ((p2 == P && p1 < P) || (p1 == P && p2 < P))
  {
    if (a.c) put(a.c + (p1 < P ? p1 : p2));
  }
  else if (p1 == P && p2 == P)
  {
    if (a.bb) put(a.bb);
  }
}

}  // namespace

int rdyn_panel_gram_pairs(int P)
{
  const int panels = (rdyn_gram_blocks_for(P) + PB - 1) / PB;
  return panels * (panels + 1) / 2;
}

// row-slice workgroups per pair: about 512 workgroups in all (two per CU), at least 4 per pair
int rdyn_panel_gram_blocks(int P)
{
  const int gx = 512 / rdyn_panel_gram_pairs(P);
  return gx < 4 ? 4 : gx;
}

size_t rdyn_panel_gram_slab_bytes(int P) { return (size_t)rdyn_panel_gram_pairs(P) * rdyn_panel_gram_blocks(P) * SLAB * sizeof(double); }

hipError_t rdyn_launch_panel_gram(const RdynPanelGramArgs& a, hipStream_t st)
{
  const dim3 grid(rdyn_panel_gram_blocks(a.P), rdyn_panel_gram_pairs(a.P));
  if (a.run_flag)
  {
    if (a.row_block > 0)
      hipLaunchKernelGGL((k_panel_gram<true, true>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((k_panel_gram<false, true>), grid, dim3(256), 0, st, a);
  }
  else if (a.row_block > 0)
    hipLaunchKernelGGL(k_panel_gram<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_panel_gram<false>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t rdyn_launch_panel_gram_finish(const RdynPanelGramArgs& a, hipStream_t st)
{
  const int pairs = rdyn_panel_gram_pairs(a.P);
  const dim3 grid((unsigned)((int64_t)pairs * SLAB / 32));
  if (a.run_flag)
    hipLaunchKernelGGL(k_panel_gram_finish<true>, grid, dim3(32 * FG), 0, st, a, pairs, rdyn_panel_gram_blocks(a.P));
  else
    hipLaunchKernelGGL(k_panel_gram_finish<false>, grid, dim3(32 * FG), 0, st, a, pairs, rdyn_panel_gram_blocks(a.P));
  return hipGetLastError();
}
