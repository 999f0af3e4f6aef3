// rdyn_image_body.inc -- body of k_image_sweep / k_image_sweep_multi (rdyn_image_impl.h), textually included (see the note in
// rdyn_local_sweep_body.inc on why it is not a __device__ function).  Expects: NJ, FIX, NT, STACKED template parameters; `a` the
// RdynSweepArgs (kernel argument, or the constant-address-space table entry of a mixed-chain plan); `blk` the index of this wave's
// 64 samples inside the batch `a` describes.
// FIX = bit mask of the chain joints that are NOT input joints (fixed joints, primitives_impl.h:74-83, and moving joints left out of
// setInputJointsName: both keep q = 0, i.e. R_pc = R_pj); the input joints are the others, in chain order: chain joint f owns row
// popcount(~FIX & ((1 << f) - 1)) of the regressor (the P' row selection of primitives_impl.h:1352).  A link hanging from a
// fixed joint still owns its ten columns (primitives_impl.h:1270: nothing is skipped).  After unrolling every use folds.
  // MAP >= 0 (FIX == 0): a.row_map[f] = the caller's row of chain joint f, -1 for MAP joints that are not input joints -- any order of
  // the input joints, fixed joints anywhere, decided at run time (wave-uniform); the sweep then carries one row per CHAIN joint (NR =
  // NJ: a fixed joint's row stays zero and is never stored) and only the image geometry (NA rows) is a compile-time figure
  constexpr int NA = MAP >= 0 ? NJ - MAP : NJ - __builtin_popcount(FIX & ((1u << NJ) - 1u));
  constexpr int NR = MAP >= 0 ? NJ : NA;             // rows the sweep carries
  constexpr int RUN = 80 * NA;                       // bytes one link adds to one sample's image
  constexpr int IMG = NJ * RUN;                      // bytes of one image
  // the image kernel flushes a link in NF pieces of CPF columns: half the ring, twice the waves per CU (the copy-out is bound
  // by LDS / store latency, not by instruction count: 3-4 waves per CU left one SIMD idle)
  constexpr int NF = STACKED ? RDYN_STACKED_FLUSHES : image_flushes(NA);
  constexpr int CPF = 10 / NF;                       // columns per flush
  constexpr int RUNF = CPF * NA * 8;                 // bytes per flush and sample
  constexpr int W = ((RUNF + 15) / 16) * 16 + 128;   // ring: one flush's run + the < 128 bytes that wait for their line
  // staging slot of one sample: the pitch in 16-byte units is ODD, so that the 8-byte staging writes of 16 consecutive lanes fall
  // on different LDS banks (2-way at worst)
  constexpr int PITCH = W + ((W / 16) % 2 ? 32 : 16);
  constexpr int MAXC = ((RUNF + 127) / 128) * 8;     // most 16-byte chunks one sample flushes at once (whole lines)
  constexpr int SPI = 64 / MAXC;                     // samples one copy-out instruction covers
  constexpr int NIT = (64 + SPI - 1) / SPI;
  extern __shared__ __attribute__((aligned(16))) char stage_wg[];
  char* const stage = stage_wg;  // one wave per workgroup: the staging area is the wave's
  ChainPtr c = as_const(a.chain);
  const int lane = threadIdx.x & 63;
  const int64_t s_wave = (int64_t)blk * 64;
  const int64_t left = a.n_samples - s_wave;
  if (left <= 0) return;  // mixed-chain plans: the grid is sized for the largest item
  const int valid = left < 64 ? (int)left : 64;
  const bool mine = lane < valid;
  const int64_t s = s_wave + (mine ? lane : 0);   // lanes past the batch idle along on the wave's first sample

  const double* __restrict__ qp = a.q + s * a.in_ss;
  const double* __restrict__ dqp = a.dq + s * a.in_ss;
  const double* __restrict__ ddqp = a.ddq + s * a.in_ss;
  // staging position of element (row l, column p of link f): image kernel -> the sample's ring, stacked -> column-major tile
  // [p][sample][row] of the link (64 NA doubles per column: exactly the bytes the wave owns in column 10 f + p of the matrix)
  char* const stg = stage + (STACKED ? lane * (NA * 8) : lane * PITCH);
  // (MAP: the image row of sweep row l is a.row_map[l], wave-uniform: one conditional subtraction instead of the folded modulo)
  int rmap[NR];
#pragma unroll
  for (int l = 0; l < NR; ++l) rmap[l] = MAP >= 0 ? a.row_map[l] : l;
  auto spos = [&](int f, int pp, int l) -> int {
    if constexpr (MAP >= 0)
    {
      const int x = (f * RUN + pp * NA * 8) % W + rmap[l] * 8;
      return x >= W ? x - W : x;
    }
    else
      return STACKED ? (pp % CPF) * (64 * NA * 8) + l * 8 : (f * RUN + (pp * NA + l) * 8) % W;
  };
  // copy-out role of this lane: chunk cj of sample (it * SPI + sub) in iteration it
  const int sub = lane / MAXC, cj = lane - sub * MAXC;
  const bool cp_lane = lane < SPI * MAXC;
  const uint32_t img = (uint32_t)(a.y_ss * 8);
  char* const ywave = (char*)(a.Y + s_wave * a.y_ss);
  // misalignment (bytes past a 128-byte line) of the image of sample (it * SPI + sub): m0 + it * dm  (mod 128)
  const uint32_t m0 = ((uint32_t)(uintptr_t)ywave + (uint32_t)sub * img) & 127u;
  const uint32_t dm = ((uint32_t)SPI * img) & 127u;
  const bool m_const = dm == 0;                      // natural strides at n = 6: every lane keeps one alignment class
  // natural stride, line-aligned wave base, full wave: the 64 images are ONE contiguous run of whole lines.  The line an image's
  // tail shares with the head of the next image is then written ONCE, whole, at the end (merge pass below) instead of as two partial
  // lines a whole sweep apart (1 line in 22.5 at n = 6, 1.75 in 30.6 at n = 7: partial lines cost a read-modify-write in HBM)
  // EXPAND (per-sample images of a chain longer than the sweep: `a.chain` is its reduced companion): the image holds the ten columns of
  // EVERY link of the full chain -- a.expand_n blocks of RUN bytes; the blocks of the links that ride on body f (a.expand_first[f] ..
  // a.expand_first[f + 1] - 1, in chain order; the links upstream of the first input joint are zero blocks) are the body's block times
  // the constant 10 x 10 blocks X_g, formed and flushed one full link at a time behind the body's kinematics
  const uint32_t IMGR = EXPAND ? (uint32_t)a.expand_n * (uint32_t)RUN : (uint32_t)IMG;  // bytes of one image
  const bool merge = !EXPAND && !STACKED && img == (uint32_t)IMG && valid == 64 && (((uint32_t)(uintptr_t)ywave) & 127u) == 0;
  double h0[10];                                     // row 0 of link 0: all that is non-zero in the first 112 bytes of an image
#pragma unroll
  for (int pp = 0; pp < 10; ++pp) h0[pp] = 0.0;
  int n_phase = 1;                                   // period of the alignment class in the copy-out iteration index
  while (((uint32_t)n_phase * dm) & 127u) ++n_phase;  // dm is a multiple of 16: at most 8

  // ---- copy-out of a per-sample-image flush: the whole lines completed by image bytes [Ep, Ec) (compile-time figures after unrolling;
  // run-time ones for the blocks of an expanded chain), everything that is left at the image's last flush
  auto flush_image = [&](const int Ep, const int Ec, const bool last) {
      // one sample's piece: x = first byte this lane moves (image offset), active if x < Fc
      auto piece = [&](uint32_t m, uint32_t j, uint32_t& x, uint32_t& pos, bool& on) {
        const uint32_t Fp = Ep == 0 ? ((merge && m) ? 128u - m : 0u) : (uint32_t)Ep - ((m + (uint32_t)Ep) & 127u);
        const uint32_t Fc = (last && !merge) ? IMGR : (uint32_t)Ec - ((m + (uint32_t)Ec) & 127u);
        x = Fp + 16u * j;
        on = x < Fc;
        // ring position of image byte x in [Ep - 127, Ec): the run starts at Ep mod W
        int pr = (int)x - Ep + (Ep % W);
        if (pr < 0) pr += W;
        if (pr >= W) pr -= W;
        pos = (uint32_t)pr;
      };
      if (cp_lane)
      {
        char* yl = ywave;  // wave-uniform, advanced by SPI images per iteration
        if (valid == 64 && m_const && 64 % SPI == 0)
        {
          uint32_t x, pos;
          bool on;
          piece(m0, (uint32_t)cj, x, pos, on);
          const uint32_t g_off = (uint32_t)sub * img + x;
          const char* const lsrc = stage + sub * PITCH + pos;
          if (on)
          {
            // a few iterations per trip: fully unrolled (NIT up to 64 per link) the kernel body outgrows what hipcc will unroll
            // over the links, and the per-link arrays of the sweep then live in scratch
#pragma unroll 4
            for (int it = 0; it < NIT; ++it)
            {
              const d2a v = *(const d2a*)(lsrc + it * (SPI * PITCH));
              if (NT) __builtin_nontemporal_store((d2u)v, (d2u*)(yl + g_off));
              else *(d2u*)(yl + g_off) = (d2u)v;
              yl += (int64_t)SPI * img;
            }
          }
        }
        else
        {
          // general strides / alignments: the misalignment of sample (it * SPI + sub) repeats with a short period in `it`
          // (n_phase <= 8: 128 / gcd(SPI * stride mod 128, 128)).  Iterations are visited phase by phase, it = ph + n_phase * k:
          // inside a phase every lane keeps ONE alignment class, so the piece arithmetic (a dozen VALU instructions) runs once
          // per phase and an iteration costs one address add, one LDS read and one store -- evaluated per iteration it took
          // 1.3 ms per 1e6 evaluations at 7 joints (3 920-byte images, eight classes) against 0.62 ms for the stacked layout.
          for (int ph = 0; ph < n_phase; ++ph)
          {
            uint32_t x, pos;
            bool on;
            piece((m0 + (uint32_t)ph * dm) & 127u, (uint32_t)cj, x, pos, on);
            const uint32_t g_off = (uint32_t)sub * img + x;
            uint32_t l_addr = (uint32_t)((ph * SPI + sub) * PITCH) + pos;
            char* yp = yl + (int64_t)ph * SPI * img;  // wave-uniform
            const int64_t g_step = (int64_t)n_phase * SPI * img;
            const uint32_t l_step = (uint32_t)(n_phase * SPI * PITCH);
            // the LDS read is unconditional (a slot past the wave's 64 reads as zeros, nothing is stored from it), so that several
            // reads of the unrolled trip are in flight: one read -> wait -> store per trip exposed the LDS latency 64 times per link
#pragma unroll 4
            for (int it = ph; it < NIT; it += n_phase)
            {
              const d2a v = *(const d2a*)(stage + l_addr);
              if (on && it * SPI + sub < valid)
              {
                if (NT) __builtin_nontemporal_store((d2u)v, (d2u*)(yp + g_off));
                else *(d2u*)(yp + g_off) = (d2u)v;
              }
              l_addr += l_step;
              yp += g_step;
            }
          }
        }
      }
      if (last)
      {
        // the image's last link can leave more than MAXC chunks (its final partial line): 8 lanes per sample pick up the rest
        const int tsub = lane >> 3, tj = MAXC + (lane & 7);
        char* yl = ywave;
#pragma unroll
        for (int it = 0; it < 8; ++it)
        {
          const int smp = it * 8 + tsub;
          const uint32_t m = ((uint32_t)(uintptr_t)ywave + (uint32_t)smp * img) & 127u;
          uint32_t x, pos;
          bool on;
          piece(m, (uint32_t)tj, x, pos, on);
          if (on && smp < valid)
          {
            const d2a v = *(const d2a*)(stage + smp * PITCH + pos);
            *(d2u*)(yl + (uint32_t)tsub * img + x) = (d2u)v;
          }
          yl += (int64_t)8 * img;
        }
      }
  };
  V3 w = mk(0, 0, 0), vl = mk(0, 0, 0), al = mk(0, 0, 0);
  V3 acc = mk(-c->g[0], -c->g[1], -c->g[2]);  // base "acceleration" -g: gravity enters every link's d for free
  V3 jl[NR], ja[NR];
  double tau[NR];
#pragma unroll
  for (int l = 0; l < NR; ++l)
  {
    tau[l] = 0.0;
    jl[l] = mk(0, 0, 0);
    ja[l] = mk(0, 0, 0);
  }

#pragma unroll
  for (int f = 0; f < NJ; ++f)
  {
    JointRef J = c->j[f];
    const int type_rt = J.type;
    const bool mov = MAP >= 0 ? rmap[f] >= 0 : !((FIX >> f) & 1u);     // input joint (pattern checked by the launcher)
    const int row = MAP >= 0 ? f : __builtin_popcount(~FIX & ((1u << f) - 1u));  // input joints upstream of f = the row joint f owns
    const int nrow = row + ((MAP >= 0 || mov) ? 1 : 0);                // rows that can be non-zero in the columns of link f + 1
    double qf = 0.0, dqf = 0.0, ddqf = 0.0;
    if (mov)
    {
      const int64_t o = (MAP >= 0 ? rmap[row] : row) * a.in_sj;
      qf = qp[o];
      dqf = dqp[o];
      ddqf = ddqp[o];
    }
    const int type = mov ? type_rt : RDYN_FIXED;  // q = 0: R_pc = R_pj, no screw
    // ---- parent -> child transform (Joint::computedTpc, primitives_impl.h:38-47)
    double R[9];
    V3 t = ld3(J.t);
    if (type == RDYN_REVOLUTE)
    {
      double sn, cs;
      rdyn_sincos(qf, &sn, &cs);
      const double oc = 1.0 - cs;
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = fma(sn, J.B[i], fma(oc, J.C[i], J.A[i]));
    }
    else
    {
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = J.A[i];
      if (type == RDYN_PRISMATIC) t = axpy(t, ld3(J.up), qf);
    }
    {
      const V3 wn = rotT(R, w);
      const V3 vn = rotT(R, vl + cross(w, t));
      const V3 aln = rotT(R, al);
      const V3 an = rotT(R, acc + cross(al, t));
      w = wn; vl = vn; al = aln; acc = an;
    }
#pragma unroll
    for (int l = 0; l < row; ++l)
    {
      const V3 nl = rotT(R, jl[l] + cross(ja[l], t));
      ja[l] = rotT(R, ja[l]);
      jl[l] = nl;
    }
    const V3 u = ld3(J.u);
    if (type == RDYN_REVOLUTE)
    {
      acc = axpy(acc, cross(vl, u), dqf);
      al = axpy(axpy(al, cross(w, u), dqf), u, ddqf);
      w = axpy(w, u, dqf);
      jl[(MAP >= 0 || mov) ? row : 0] = mk(0, 0, 0);  // (type is RDYN_FIXED unless mov)
      ja[(MAP >= 0 || mov) ? row : 0] = u;
    }
    else if (type == RDYN_PRISMATIC)
    {
      acc = axpy(axpy(acc, cross(w, u), dqf), u, ddqf);
      vl = axpy(vl, u, dqf);
      jl[(MAP >= 0 || mov) ? row : 0] = u;
      ja[(MAP >= 0 || mov) ? row : 0] = mk(0, 0, 0);
    }
    // ---- closed-form wrench regressor of link f + 1 in its own frame, rows of the input joints l <= f
    const V3 d = acc + cross(w, vl);
    const double wxy = w.x * w.y, wxz = w.x * w.z, wyz = w.y * w.z;
    const double wxx = w.x * w.x, wyy = w.y * w.y, wzz = w.z * w.z;
    const double b00 = -(wyy + wzz), b01 = wxy - al.z, b02 = wxz + al.y;
    const double b10 = wxy + al.z, b11 = -(wxx + wzz), b12 = wyz - al.x;
    const double b20 = wxz - al.y, b21 = wyz + al.x, b22 = -(wxx + wyy);
    const RDYN_CONST_AS double* pi = J.pi;
    // the ten-vector of row l in link f + 1 (rows l <= f)
    auto row_y = [&](int l, double (&y)[10]) {
      const V3 L = jl[l], A = ja[l];
      const V3 dxA = cross(d, A);
      const V3 x = cross(A, w);
      y[0] = dot(L, d);
      y[1] = fma(L.x, b00, fma(L.y, b10, fma(L.z, b20, dxA.x)));
      y[2] = fma(L.x, b01, fma(L.y, b11, fma(L.z, b21, dxA.y)));
      y[3] = fma(L.x, b02, fma(L.y, b12, fma(L.z, b22, dxA.z)));
      y[4] = fma(A.x, al.x, x.x * w.x);
      y[5] = fma(A.x, al.y, fma(A.y, al.x, fma(x.x, w.y, x.y * w.x)));
      y[6] = fma(A.x, al.z, fma(A.z, al.x, fma(x.x, w.z, x.z * w.x)));
      y[7] = fma(A.y, al.y, x.y * w.y);
      y[8] = fma(A.y, al.z, fma(A.z, al.y, fma(x.y, w.z, x.z * w.y)));
      y[9] = fma(A.z, al.z, x.z * w.z);
    };
    if constexpr (EXPAND)
    {
      static_assert(!EXPAND || (NF == 1 && !STACKED && MAP == 0), "expanded images: one flush per link block, row map");
      // the torque of the body's joints: its own block times its parameters, once
#pragma unroll
      for (int l = 0; l < NR; ++l)
        if (l < nrow)
        {
          double y[10];
          row_y(l, y);
          double tl = tau[l];
#pragma unroll
          for (int p = 0; p < 10; ++p) tl = fma(y[p], pi[p], tl);
          asm volatile("" : "+v"(tl));
          tau[l] = tl;
        }
      const int g_first = a.expand_first[0];
      const int g_lo = f == 0 ? 0 : a.expand_first[f], g_hi = a.expand_first[f + 1];
      for (int g = g_lo; g < g_hi; ++g)  // wave-uniform
      {
        const bool rides = g >= g_first;  // (false: a link upstream of the first input joint -- a zero block; f == 0 only)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
        const RDYN_CONST_AS double* X = (const RDYN_CONST_AS double*)a.expand_X + g * 100;
#pragma clang diagnostic pop
        const int Eg = g * RUN, base = Eg % W;
        // rows in two halves: a half's ten-vectors and results are what stays in registers (60 + 60 at six rows: all of them at once is
        // the 256-register shape of k_expand_staged)
        constexpr int HR = (NR + 1) / 2;
#pragma unroll
        for (int h = 0; h < 2; ++h)
        {
          double yh[HR][10], oh[HR][10];
#pragma unroll
          for (int i = 0; i < HR; ++i)
          {
            const int l = h * HR + i;
#pragma unroll
            for (int p = 0; p < 10; ++p) yh[i][p] = oh[i][p] = 0.0;
            if (l < NR && l < nrow && rides) row_y(l, yh[i]);
          }
          if (rides)
          {
#pragma unroll
            for (int e = 0; e < 10; ++e)
            {
              double xe[10];
#pragma unroll
              for (int p = 0; p < 10; ++p) xe[p] = X[e * 10 + p];
#pragma unroll
              for (int i = 0; i < HR; ++i)
                if (h * HR + i < NR && h * HR + i < nrow)
                {
#pragma unroll
                  for (int p = 0; p < 10; ++p) oh[i][p] = fma(yh[i][e], xe[p], oh[i][p]);
                }
            }
          }
#pragma unroll
          for (int i = 0; i < HR; ++i)
          {
            const int l = h * HR + i;
            if (l >= NR) continue;
#pragma unroll
            for (int p = 0; p < 10; ++p)
            {
              int x = base + (p * NA + rmap[l]) * 8;
              x = x >= W ? x - W : x;
              *(double*)(stg + x) = oh[i][p];
            }
          }
        }
        wave_lds_fence();
        flush_image(Eg, Eg + RUN, g == a.expand_n - 1);
        wave_lds_fence();
      }
    }
    else
    {
#pragma unroll
    for (int hf = 0; hf < NF; ++hf)
    {
    const int p_lo = hf * CPF, p_hi = p_lo + CPF;  // this flush's columns (the other columns' arithmetic is dead code here)
#pragma unroll
    for (int l = 0; l < NR; ++l)
    {
      if (MAP > 0 && rmap[l] < 0) continue;  // the row of a joint that is not an input joint: not in the image
      if (l < nrow)
      {
        double y[10];
        row_y(l, y);
        double tl = tau[l];
#pragma unroll
        for (int p = 0; p < 10; ++p)
        {
          if (p < p_lo || p >= p_hi) continue;
          tl = fma(y[p], pi[p], tl);
          *(double*)(stg + spos(f, p, l)) = y[p];
          if (!STACKED && f == 0 && l == 0) h0[p] = y[p];
        }
        // pin the running torque here: tau is only read in the conditional store at the very end, and LLVM otherwise SINKS the last
        // links' y * pi chains into that block, keeping their sixty y values alive (and spilled) across the copy-out
        asm volatile("" : "+v"(tl));
        tau[l] = tl;
      }
      else
      {
        // structural zero block (row of a joint downstream of this link): the image is dense
#pragma unroll
        for (int p = 0; p < 10; ++p)
          if (p >= p_lo && p < p_hi) *(double*)(stg + spos(f, p, l)) = 0.0;
      }
    }
    // ---- copy out the lines completed by this link: image bytes [Fp, Fc), Fx = E - ((m + E) mod 128) (everything at the last link)
    wave_lds_fence();
    if constexpr (STACKED)
    {
      // the wave owns 64 NA consecutive doubles of every column: 512 NA bytes = 4 NA whole lines when the column is line aligned
      const uint32_t lim = (uint32_t)valid * (NA * 8);
#pragma unroll
      for (int pq = 0; pq < CPF; ++pq)
      {
        const int pp = p_lo + pq;
        char* const ycol = (char*)(a.Y + (int64_t)(10 * f + pp) * a.y_sc + s_wave * NA);  // wave-uniform
#pragma unroll
        for (int it = 0; it < (32 * NA + 63) / 64; ++it)
        {
          const uint32_t off = (uint32_t)(it * 64 + lane) * 16u;
          if (off < lim)
          {
            const d2a v = *(const d2a*)(stage + pq * (64 * NA * 8) + off);
            if (off + 16u <= lim)
            {
              if (NT) __builtin_nontemporal_store((d2u)v, (d2u*)(ycol + off));
              else *(d2u*)(ycol + off) = (d2u)v;
            }
            else
              *(double*)(ycol + off) = v.x;  // odd number of valid doubles: the last chunk is half full
          }
        }
      }
    }
    else
    {
      flush_image(f * RUN + hf * RUNF, f * RUN + hf * RUNF + RUNF, f == NJ - 1 && hf == NF - 1);
    }
    wave_lds_fence();  // the ring is written again by the next flush
    }
    }  // (!EXPAND)
  }
  if constexpr (!STACKED)
  {
    if (merge)
    {
      // ---- the lines shared by two images: [tail of image l | head of image l + 1], written whole, once
      const uint32_t m_l = ((uint32_t)lane * (uint32_t)IMG) & 127u;          // my image starts m_l bytes into a line
      const uint32_t tail = (m_l + (uint32_t)IMG) & 127u;                      // bytes of my image in the line it ends in (0: none)
      d2a t[7];
#pragma unroll
      for (int ch = 0; ch < 7; ++ch)
      {
        t[ch] = (d2a){0.0, 0.0};
        if (16u * ch < tail) t[ch] = *(const d2a*)(stg + ((uint32_t)IMG - tail + 16u * ch) % (uint32_t)W);  // ring position = image offset mod W
      }
      wave_lds_fence();
#pragma unroll
      for (int ch = 0; ch < 7; ++ch)
        if (16u * ch < tail) *(d2a*)(stg + 16 * ch) = t[ch];
      if (m_l)  // my head completes the previous image's line (lane > 0: the wave's base is line-aligned)
      {
        char* const dst = stage + (lane - 1) * PITCH + m_l;
#pragma unroll
        for (int i = 0; i < 14; ++i)
          if (8u * i < 128u - m_l) *(double*)(dst + 8 * i) = (i % NA == (MAP >= 0 ? rmap[0] : 0) && i / NA < 10) ? h0[i / NA < 10 ? i / NA : 0] : 0.0;
      }
      wave_lds_fence();
      const int tsub = lane >> 3, tj = lane & 7;
      char* yl = ywave;
#pragma unroll
      for (int it = 0; it < 8; ++it)
      {
        const int smp = it * 8 + tsub;
        const uint32_t tl_s = (((uint32_t)smp + 1u) * (uint32_t)IMG) & 127u;  // tail of image smp
        if (tl_s)
        {
          const d2a v = *(const d2a*)(stage + smp * PITCH + 16 * tj);
          if (NT) __builtin_nontemporal_store((d2u)v, (d2u*)(yl + (uint32_t)tsub * img + ((uint32_t)IMG - tl_s) + 16u * tj));
          else *(d2u*)(yl + (uint32_t)tsub * img + ((uint32_t)IMG - tl_s) + 16u * tj) = (d2u)v;
        }
        yl += (int64_t)8 * img;
      }
    }
  }
  if (a.tau && mine)
  {
    double* __restrict__ tp = a.tau + s * a.tau_ss;
#pragma unroll
    for (int l = 0; l < NR; ++l)
      if (MAP <= 0 || rmap[l] >= 0) tp[(MAP >= 0 ? rmap[l] : l) * a.tau_sj] = tau[l];
  }
