// IPCS: the register-resident pressure solvers of mode 3 (cg_pressure_reg, cg_pressure_regm_w, cg_pressure_regm,
// cg_pressure_cheb, cg_pressure_2l).  Included by mdq_ipcs.hip (the entry unit) only, behind cg_pressure.
namespace mdq {

// Jacobi-scaled CG on the SELL-64 P1 Laplacian for the three-kernel mode 3: every thread keeps x, r, q of its own
// two rows (slice = wave, wave + NTH/64; lane = row in the slice: the rows its SpMV produces) in registers, only the
// search direction lives in LDS for the gather; one-barrier reductions.  3 barriers per iteration instead of 6.
// Needs n <= 2 * NTH (the caller falls back to cg_pressure otherwise).  x, r, p: LDS vectors as in cg_pressure.
template <int NTH>
__device__ inline int cg_pressure_reg(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A, double rtol,
                                      int maxit, double* x, double* r, double* p, double* red, int& rsel) {
  constexpr int NW = NTH / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nsl = (n + 63) >> 6;
  int base[2], wid[2], row[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int s_ = wave + NW * k;
    row[k] = (s_ << 6) + lane;
    base[k] = s_ < nsl ? sl_off[s_] : 0;
    wid[k] = s_ < nsl ? (sl_off[s_ + 1] - base[k]) >> 6 : 0;
  }
  auto spmv = [&](const double* vec, double(&y)[2]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double* a = A + base[k] + lane;
      const int32_t* c = sl_col + base[k] + lane;
      double y0 = 0.0;
#pragma unroll 4
      for (int j = 0; j < wid[k]; ++j) y0 += a[j * 64] * vec[c[j * 64]];
      y[k] = y0;
    }
  };
  __syncthreads();
  double y[2], xv[2], rv[2], pv[2];
  spmv(x, y);
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    xv[k] = rv[k] = pv[k] = 0.0;
    if (row[k] < n) {
      const double b = r[row[k]];
      xv[k] = x[row[k]];
      rv[k] = pv[k] = b - y[k];
      p[row[k]] = pv[k];
      acc[0] += b * b;
      acc[1] += rv[k] * rv[k];
    }
  }
  block_sum<2, NW>(acc, red);
  const double bb = acc[0], tol2 = rtol * rtol * bb;
  double rr = acc[1];
  int it = 0;
  if (rr > tol2 && bb != 0.0) {
    while (it < maxit) {
      ++it;
      double q[2];
      spmv(p, q);
      double a1[1] = {pv[0] * q[0] + pv[1] * q[1]};
      block_sum1<1, NW>(a1, red, rsel);
      if (!(a1[0] > 0.0)) break;
      const double alpha = rr / a1[0];
      double a2[1] = {0.0};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        xv[k] += alpha * pv[k];
        rv[k] -= alpha * q[k];
        a2[0] += rv[k] * rv[k];
      }
      block_sum1<1, NW>(a2, red, rsel);
      const double rr_new = a2[0];
      if (!(rr_new > tol2)) break;
      const double beta = rr_new / rr;
      rr = rr_new;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        pv[k] = rv[k] + beta * pv[k];
        if (row[k] < n) p[row[k]] = pv[k];
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (row[k] < n) x[row[k]] = xv[k];
  __syncthreads();
  return it;
}

// cg_pressure_reg with the matrix rows of a thread in REGISTERS and a BRANCH-FREE operator application.  Counters of the
// LDS-resident version (profiles/r03_sq_summary.json): LDS utilisation 20 %, bank conflicts 0.3 %, VALU busy 18 % - the
// iteration is a chain of LDS LATENCIES, not bandwidth: per row three batches of (index, value) reads followed by the
// dependent gathers, two rows one after the other, ~2 100 of the iteration's ~3 400 cycles.  Here a thread loads the
// up to RW entries of its two rows once (slots past a slice's width: value 0, column = own row, like the SELL padding),
// and an application issues all 2 x RW gathers back to back - no branch, so nothing waits between them - and then runs
// the two fma chains in the same column order as before (adding 0 * p[row] for the padded slots).  (The Chebyshev
// variant below keeps its rows in registers too but guards every gather with a branch on the slice width, which
// serialises the round trips: that is why it never beat the LDS version.)  Needs n <= 2 * NTH and slices of at most RW
// entries per row.
//
// RW is the number of register slots per row.  The solve is instantiated at 10, 12 and 16 and the caller
// (cg_pressure_regm below) takes the smallest that holds the environment's widest slice: the P1 Laplacian of the lab
// meshes has rows of at most 9 entries (SELL-64 slice widths 6-9), so at RW = 16 twelve to fourteen of the 32 gathers of an
// application read the thread's own row and multiply it by zero.  The dropped slots have value 0 and sit behind every real
// entry of the row: the fma chain ends with acc + 0 * p[row] = acc there, so every iterate, every reduction and the
// iteration count are those of RW = 16, bit for bit.  The caller guarantees that every slice is at most RW wide.
template <int NTH, int RW>
__device__ inline int cg_pressure_regm_w(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A, double rtol,
                                         int maxit, double* x, double* r, double* p, double* red, int& rsel) {
  constexpr int NW = NTH / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nsl = (n + 63) >> 6;
  int row[2];
  double av[2][RW];
  int co[2][RW];                      // byte offsets into the gathered vector
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int s_ = wave + NW * k;
    row[k] = (s_ << 6) + lane;
    const int base = s_ < nsl ? sl_off[s_] : 0;
    const int wid = s_ < nsl ? (sl_off[s_ + 1] - base) >> 6 : 0;
    const int self = min(row[k], n - 1);
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      const bool in = j < wid;
      av[k][j] = in ? A[base + lane + j * 64] : 0.0;
      co[k][j] = 8 * (in ? sl_col[base + lane + j * 64] : self);
    }
  }
  auto spmv = [&](const double* vec, double(&y)[2]) {
    const char* vb = reinterpret_cast<const char*>(vec);
    double g[2][RW];
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      g[0][j] = *reinterpret_cast<const double*>(vb + co[0][j]);
      g[1][j] = *reinterpret_cast<const double*>(vb + co[1][j]);
    }
    double y0 = 0.0, y1 = 0.0;
#pragma unroll
    for (int j = 0; j < RW; ++j) {
      y0 += av[0][j] * g[0][j];
      y1 += av[1][j] * g[1][j];
    }
    y[0] = y0;
    y[1] = y1;
  };
  __syncthreads();
  double y[2], xv[2], rv[2], pv[2];
  spmv(x, y);
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    xv[k] = rv[k] = pv[k] = 0.0;
    if (row[k] < n) {
      const double b = r[row[k]];
      xv[k] = x[row[k]];
      rv[k] = pv[k] = b - y[k];
      p[row[k]] = pv[k];
      acc[0] += b * b;
      acc[1] += rv[k] * rv[k];
    }
  }
  block_sum<2, NW>(acc, red);
  const double bb = acc[0], tol2 = rtol * rtol * bb;
  double rr = acc[1];
  int it = 0;
  if (rr > tol2 && bb != 0.0) {
    while (it < maxit) {
      ++it;
      double q[2];
      spmv(p, q);
      double a1[1] = {pv[0] * q[0] + pv[1] * q[1]};
      block_sum1<1, NW>(a1, red, rsel);
      if (!(a1[0] > 0.0)) break;
      const double alpha = rr / a1[0];
      double a2[1] = {0.0};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        xv[k] += alpha * pv[k];
        rv[k] -= alpha * q[k];
        a2[0] += rv[k] * rv[k];
      }
      block_sum1<1, NW>(a2, red, rsel);
      const double rr_new = a2[0];
      if (!(rr_new > tol2)) break;
      const double beta = rr_new / rr;
      rr = rr_new;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        pv[k] = rv[k] + beta * pv[k];
        if (row[k] < n) p[row[k]] = pv[k];
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (row[k] < n) x[row[k]] = xv[k];
  __syncthreads();
  return it;
}

// cg_pressure_regm_w at the environment's width.  Every thread reads ALL slice offsets (at most 2 * NTH / 64 + 1 words,
// the same addresses in every lane), so the widest slice - and with it the variant - is the same value in every thread of
// the workgroup without a reduction: the barriers inside the variants are reached by all waves or by none.
template <int NTH>
__device__ inline int cg_pressure_regm(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A, double rtol,
                                       int maxit, double* x, double* r, double* p, double* red, int& rsel) {
  const int nsl = (n + 63) >> 6;
  int wmax = 0, o0 = sl_off[0];
  for (int s_ = 0; s_ < nsl; ++s_) {
    const int o1 = sl_off[s_ + 1];
    wmax = max(wmax, (o1 - o0) >> 6);
    o0 = o1;
  }
  wmax = __builtin_amdgcn_readfirstlane(wmax);
  if (wmax <= 10) return cg_pressure_regm_w<NTH, 10>(n, sl_off, sl_col, A, rtol, maxit, x, r, p, red, rsel);
  if (wmax <= 12) return cg_pressure_regm_w<NTH, 12>(n, sl_off, sl_col, A, rtol, maxit, x, r, p, red, rsel);
  if (wmax <= 16) return cg_pressure_regm_w<NTH, 16>(n, sl_off, sl_col, A, rtol, maxit, x, r, p, red, rsel);
  return -1;
}

// The same CG with the matrix rows of a thread in REGISTERS (values + column offsets of its two rows: they do not change
// over the iterations, and the LDS-resident version paid two dependent LDS round trips per entry - column, then vector
// element) and, for degree > 1, a CHEBYSHEV polynomial preconditioner on top of the Jacobi scaling: z = p_m(A) r with
// p_m the degree-(m - 1) Chebyshev approximation of 1 / lambda on [lmax / CHEB_RATIO, lmax] (lmax: Gershgorin bound of the
// scaled matrix, computed here).  p_m(A) is symmetric positive definite for any spectrum inside (0, lmax], so this is a
// plain preconditioned CG; it trades reductions (two workgroup barriers each) for operator applications (one barrier):
// m - 1 extra applications per iteration, roughly m times fewer iterations.  Needs n <= 2 * NTH and SELL slices of at
// most PCG_W entries per row (else: returns -1 and the caller takes cg_pressure_reg).
constexpr int PCG_W = 12;
constexpr double CHEB_RATIO = 30.0;
template <int NTH>
__device__ inline int cg_pressure_cheb(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A, double rtol,
                                       int maxit, int degree, double* x, double* r, double* p, double* red, int& rsel) {
  constexpr int NW = NTH / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nsl = (n + 63) >> 6;
  int row[2], wid[2];
  double av[2][PCG_W];
  int cv[2][PCG_W];
  bool fits = true;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int s_ = wave + NW * k;
    row[k] = (s_ << 6) + lane;
    const int base = s_ < nsl ? sl_off[s_] : 0;
    wid[k] = s_ < nsl ? (sl_off[s_ + 1] - base) >> 6 : 0;
    fits = fits && wid[k] <= PCG_W;
#pragma unroll
    for (int j = 0; j < PCG_W; ++j) {
      const bool in = j < wid[k];
      av[k][j] = in ? A[base + lane + j * 64] : 0.0;
      cv[k][j] = in ? sl_col[base + lane + j * 64] : 0;
    }
  }
  // workgroup-wide OR of `!fits` through the (still unused) search-direction vector: __syncthreads_or would add a static
  // LDS word to kernels that already ask for the whole 160 KB dynamically
  if (threadIdx.x == 0) p[NW] = 0.0;
  __syncthreads();
  if (!fits) p[NW] = 1.0;
  __syncthreads();
  const bool toowide = p[NW] != 0.0;
  __syncthreads();
  if (toowide) return -1;
  auto spmv = [&](const double* vec, double(&y)[2]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double y0 = 0.0, y1 = 0.0;
#pragma unroll
      for (int j = 0; j < PCG_W; j += 2) {
        if (j < wid[k]) y0 += av[k][j] * vec[cv[k][j]];            // (wid is uniform over the wave: scalar branches)
        if (j + 1 < wid[k]) y1 += av[k][j + 1] * vec[cv[k][j + 1]];
      }
      y[k] = y0 + y1;
    }
  };
  // Gershgorin bound of the largest eigenvalue (the scaled matrix has a unit diagonal; rows of constrained vertices are
  // identity rows)
  double lmax = 0.0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    double s_ = 0.0;
#pragma unroll
    for (int j = 0; j < PCG_W; ++j) s_ += fabs(av[k][j]);
    lmax = fmax(lmax, row[k] < n ? s_ : 0.0);
  }
  for (int off = 32; off > 0; off >>= 1) lmax = fmax(lmax, __shfl_xor(lmax, off));
  {
    double* buf = p;                          // (the search direction is not in use yet)
    if (lane == 0) buf[wave] = lmax;
    __syncthreads();
    double m_ = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) m_ = fmax(m_, buf[i]);
    lmax = m_;
    __syncthreads();
  }
  const int M = degree < 1 ? 1 : degree;
  const double lmin = lmax / CHEB_RATIO, theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
  double y[2], xv[2], rv[2], pv[2], zv[2];
  spmv(x, y);
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    xv[k] = rv[k] = pv[k] = zv[k] = 0.0;
    if (row[k] < n) {
      const double b = r[row[k]];
      xv[k] = x[row[k]];
      rv[k] = b - y[k];
      acc[0] += b * b;
      acc[1] += rv[k] * rv[k];
    }
  }
  block_sum<2, NW>(acc, red);
  const double bb = acc[0], tol2 = rtol * rtol * bb;
  double rr = acc[1];
  int it = 0;
  if (rr > tol2 && bb != 0.0) {
    double rz_old = 1.0;
    // `r` (LDS) is free from here on: the polynomial's iterates are staged there for the gathers
    double* zs = r;
    while (it < maxit) {
      // z = p_M(A) r  (Chebyshev iteration for A z = r from z = 0, M - 1 further applications)
      double dv[2];
      double rho = 1.0 / sigma;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        dv[k] = rv[k] / theta;
        zv[k] = dv[k];
      }
      for (int m_ = 1; m_ < M; ++m_) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (row[k] < n) zs[row[k]] = zv[k];
        __syncthreads();
        double az[2];
        spmv(zs, az);
        const double rho_n = 1.0 / (2.0 * sigma - rho);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          dv[k] = rho_n * rho * dv[k] + (2.0 * rho_n / delta) * (rv[k] - az[k]);
          zv[k] += dv[k];
        }
        rho = rho_n;
        __syncthreads();                         // (everybody has gathered from zs before the next round rewrites it)
      }
      double a0[1] = {rv[0] * zv[0] + rv[1] * zv[1]};
      block_sum1<1, NW>(a0, red, rsel);
      const double rz = a0[0];
      const double beta = it == 0 ? 0.0 : rz / rz_old;
      rz_old = rz;
      ++it;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        pv[k] = zv[k] + beta * pv[k];
        if (row[k] < n) p[row[k]] = pv[k];
      }
      __syncthreads();
      double q[2];
      spmv(p, q);
      double a1[1] = {pv[0] * q[0] + pv[1] * q[1]};
      block_sum1<1, NW>(a1, red, rsel);
      if (!(a1[0] > 0.0)) break;
      const double alpha = rz / a1[0];
      double a2[1] = {0.0};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        xv[k] += alpha * pv[k];
        rv[k] -= alpha * q[k];
        a2[0] += rv[k] * rv[k];
      }
      block_sum1<1, NW>(a2, red, rsel);
      rr = a2[0];
      if (!(rr > tol2)) break;
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (row[k] < n) x[row[k]] = xv[k];
  __syncthreads();
  return it;
}

// The register-resident CG (cg_pressure_reg) with a TWO-LEVEL additive preconditioner on top of the Jacobi scaling:
//      z = r + P A_c^-1 P^T r,     A_c = P^T A P,
// P = piecewise constants over NAGX x NAGY geometric aggregates: vertices ranked by x into NAGX strips of equal
// population, every strip ranked by y into NAGY cells (compact patches of ~16 vertices; aggregates of consecutive INDICES
// do nothing for this matrix: tools + HISTORY 8.1).  A_c (56 x 56) is accumulated with LDS atomics, inverted in LDS by
// Gauss-Jordan (SPD: no pivoting) once per solve and kept in fp32 (a preconditioner may be approximate; it is stored
// exactly symmetric).  Per iteration: per-wave partial restrictions by LDS atomics (rows of one aggregate are scattered
// over the waves), one 56^2 product spread over 448 threads, prolongation by one LDS read per row: two extra barriers.
// Iterations on ys930 (developed flow): 154 -> 86, same answers.  MEASURED (tools/time_pcg.py): 465 us per solve against 247 us of
// the plain Jacobi-CG - the O(n^2) rank counts of the aggregation and the 56-step inversion cost ~0.1 ms per solve, and
// every iteration pays two more barriers, the atomics and a 63-read coarse product per thread.  An O(n) aggregation
// (histograms) and one shared restriction vector would bring it to ~200 us (-18 %): kept as an OPTION (pcg_degree < 0), the
// default stays the Jacobi-CG.  LDS: the four pressure vectors' space (x, r, p, q = 4 NVp doubles, NVp >= 1024):
// x and r live in registers during the iterations.  Needs n <= 2 NTH, n <= 1024 and at least NAG vertices; else -1.
template <int NTH>
__device__ inline int cg_pressure_2l(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A, const double* coords,
                                     double rtol, int maxit, double* x, double* r, double* p, int NVp, double* red, int& rsel) {
  constexpr int NW = NTH / 64;
  if (n > 2 * NTH || n > 1024 || n < 4 * NAG || NVp < 1024) return -1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nsl = (n + 63) >> 6;
  int base[2], wid[2], row[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int s_ = wave + NW * k;
    row[k] = (s_ << 6) + lane;
    base[k] = s_ < nsl ? sl_off[s_] : 0;
    wid[k] = s_ < nsl ? (sl_off[s_ + 1] - base[k]) >> 6 : 0;
  }
  auto spmv = [&](const double* vec, double(&y)[2]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double* a = A + base[k] + lane;
      const int32_t* c = sl_col + base[k] + lane;
      double y0 = 0.0;
#pragma unroll 4
      for (int j = 0; j < wid[k]; ++j) y0 += a[j * 64] * vec[c[j * 64]];
      y[k] = y0;
    }
  };
  // LDS carve-up of the 4 NVp doubles behind x (x | r | p | q are contiguous in every caller)
  double* W = x;
  double* AC = W;                                            // [NAG][NAG] fp64 while it is built and inverted
  float* AI = reinterpret_cast<float*>(W);                   // ... then fp32 in its first half
  double* YV = W + NAG * NAG / 2 + 8;                        // [NAG] coarse result       (behind the fp32 inverse)
  double* PG = W + 2 * NVp;                                  // the gather copy of the search direction (= p)
  double* WP = W + 3 * NVp;                                  // [NW][NAG] per-wave partial restrictions
  unsigned char* AG = reinterpret_cast<unsigned char*>(W + 3 * NVp + NW * NAG);   // [n] aggregate of a vertex
  static_assert(NAG * NAG <= 3 * 1024 + 64 && 16 * NAG + 128 <= 1024, "two-level scratch");
  __syncthreads();
  double y[2], xv[2], rv[2], pv[2], zv[2];
  spmv(x, y);
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    xv[k] = rv[k] = pv[k] = zv[k] = 0.0;
    if (row[k] < n) {
      const double b = r[row[k]];
      xv[k] = x[row[k]];
      rv[k] = b - y[k];
      acc[0] += b * b;
      acc[1] += rv[k] * rv[k];
    }
  }
  block_sum<2, NW>(acc, red);                                // (its barriers: x and r are in registers, their LDS space is free)
  const double bb = acc[0], tol2 = rtol * rtol * bb;
  double rr = acc[1];
  int it = 0;
  if (rr > tol2 && bb != 0.0) {
    // ---- aggregates: rank by x -> strip, rank by y inside the strip -> cell
    double* XC = W;                                          // coordinates staged in LDS for the counting loops
    double* YC = W + 1024;
    unsigned char* ST = reinterpret_cast<unsigned char*>(W + 2048);
    for (int i = tid; i < n; i += NTH) {
      XC[i] = coords[2 * i];
      YC[i] = coords[2 * i + 1];
    }
    __syncthreads();
    int strip[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (row[k] < n) {
        const double xi = XC[row[k]];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
          const double xj = XC[j];
          rank += (xj < xi) | ((xj == xi) & (j < row[k]));
        }
        strip[k] = rank * NAGX / n;
        ST[row[k]] = (unsigned char)strip[k];
      }
    __syncthreads();
    int agg[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (row[k] < n) {
        const double yi = YC[row[k]];
        int rank = 0, cnt = 0;
        for (int j = 0; j < n; ++j) {
          const bool same = ST[j] == strip[k];
          const double yj = YC[j];
          cnt += same;
          rank += same & ((yj < yi) | ((yj == yi) & (j < row[k])));
        }
        agg[k] = strip[k] * NAGY + rank * NAGY / cnt;
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (row[k] < n) AG[row[k]] = (unsigned char)agg[k];
    for (int e = tid; e < NAG * NAG; e += NTH) AC[e] = 0.0;
    __syncthreads();
    // ---- coarse matrix
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (row[k] < n) {
        const double* a = A + base[k] + lane;
        const int32_t* c = sl_col + base[k] + lane;
        for (int j = 0; j < wid[k]; ++j) {
          const double av = a[j * 64];
          if (av != 0.0) atomicAdd(&AC[agg[k] * NAG + AG[c[j * 64]]], av);
        }
      }
    __syncthreads();
    // ---- in-place Gauss-Jordan inverse (every thread owns the elements e = tid + m NTH)
    constexpr int EPT = (NAG * NAG + NTH - 1) / NTH;
    int ei_[EPT], ej_[EPT];
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
      const int e = tid + m * NTH;
      ei_[m] = e / NAG;
      ej_[m] = e - ei_[m] * NAG;
    }
    for (int kk = 0; kk < NAG; ++kk) {
      const double ip = 1.0 / AC[kk * NAG + kk];
      double nv_[EPT];
#pragma unroll
      for (int m = 0; m < EPT; ++m) {
        const int e = tid + m * NTH;
        nv_[m] = 0.0;
        if (e < NAG * NAG) {
          const int i = ei_[m], j = ej_[m];
          const double aij = AC[e], aik = AC[i * NAG + kk], akj = AC[kk * NAG + j];
          nv_[m] = i == kk ? (j == kk ? ip : akj * ip) : (j == kk ? -aik * ip : aij - aik * akj * ip);
        }
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < EPT; ++m) {
        const int e = tid + m * NTH;
        if (e < NAG * NAG) AC[e] = nv_[m];
      }
      __syncthreads();
    }
    {  // fp32 copy, exactly symmetric: the entry of the upper triangle for both (i, j) and (j, i)
      float f_[EPT];
#pragma unroll
      for (int m = 0; m < EPT; ++m) {
        const int e = tid + m * NTH;
        f_[m] = 0.f;
        if (e < NAG * NAG) {
          const int i = e / NAG, j = e - i * NAG;
          f_[m] = (float)AC[min(i, j) * NAG + max(i, j)];
        }
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < EPT; ++m) {
        const int e = tid + m * NTH;
        if (e < NAG * NAG) AI[e] = f_[m];
      }
    }
    __syncthreads();
    double rz_old = 1.0;
    while (it < maxit) {
      // ---- z = r + P A_c^-1 P^T r
      if (lane < NAG) WP[wave * NAG + lane] = 0.0;
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (row[k] < n) atomicAdd(&WP[wave * NAG + agg[k]], rv[k]);
      __syncthreads();
      if (tid < NAG * 8) {
        const int I = tid >> 3, part = tid & 7;
        double s_ = 0.0;
        for (int J = part; J < NAG; J += 8) {
          double w_ = 0.0;
#pragma unroll
          for (int q = 0; q < NW; ++q) w_ += WP[q * NAG + J];
          s_ += (double)AI[I * NAG + J] * w_;
        }
        s_ += dpp_get<0xB1, 0xF>(s_);      // quad_perm [1,0,3,2]
        s_ += dpp_get<0x4E, 0xF>(s_);      // quad_perm [2,3,0,1]
        s_ += dpp_get<0x141, 0xF>(s_);     // row_half_mirror: the other quad of the group of 8
        if (part == 0) YV[I] = s_;
      }
      __syncthreads();
      double a0[1] = {0.0};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        zv[k] = row[k] < n ? rv[k] + YV[agg[k]] : 0.0;
        a0[0] += rv[k] * zv[k];
      }
      block_sum1<1, NW>(a0, red, rsel);
      const double rz = a0[0];
      const double beta = it == 0 ? 0.0 : rz / rz_old;
      rz_old = rz;
      ++it;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        pv[k] = zv[k] + beta * pv[k];
        if (row[k] < n) PG[row[k]] = pv[k];
      }
      __syncthreads();
      double q[2];
      spmv(PG, q);
      double a1[1] = {pv[0] * q[0] + pv[1] * q[1]};
      block_sum1<1, NW>(a1, red, rsel);
      if (!(a1[0] > 0.0)) break;
      const double alpha = rz / a1[0];
      double a2[1] = {0.0};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        xv[k] += alpha * pv[k];
        rv[k] -= alpha * q[k];
        a2[0] += rv[k] * rv[k];
      }
      block_sum1<1, NW>(a2, red, rsel);
      rr = a2[0];
      if (!(rr > tol2)) break;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (row[k] < n) x[row[k]] = xv[k];
  __syncthreads();
  return it;
}

}  // namespace mdq
