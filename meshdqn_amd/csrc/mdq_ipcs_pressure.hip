// IPCS, shared: the two-level pressure CG, pressure_krylov_lds, the buffers and macros of the MDQ_AT_TRACE stamps and the
// direct pressure solve.  Included by all four IPCS units, behind the Krylov solvers (the entry unit: behind mdq_ipcs_pcg_reg.hip).
namespace mdq {

// The two-level preconditioner for the meshes BEYOND the register-resident solvers (cg_pressure: four LDS vectors, 512
// threads, any n up to the LDS): where Jacobi-CG needs hundreds of iterations (refined ys930, 3 322 vertices: 320-343).
// Same operator z = r + P A_c^-1 P^T r over NAGX x NAGY geometric aggregates as cg_pressure_2l, with what that one's header
// lists as missing: the aggregation in O(n) - a 1 024-bin histogram of x, its prefix sums cut into NAGX strips of (about)
// equal population, per strip a 256-bin histogram of y cut into NAGY cells; vertices of one fine bin share a strip / cell,
// an empty aggregate gets a unit diagonal - and one-barrier reductions.  Scratch: the histograms and then the fp64 coarse
// matrix in the p | q vectors (free until the first search direction), the fp32 inverse, the per-wave partial
// restrictions and the aggregate of every vertex in `extra` (LDS: the fifth pressure vector, the direct solver's scratch).
// The four CG vectors may as well live in GLOBAL memory (meshes beyond ~4 000 vertices, the PG instances of the kernels:
// `scratch` is then the search direction's slab vector, `extra` the LDS the pressure vectors do not occupy).
// Returns -1 where it does not apply (too few vertices, a scratch too small): the caller runs cg_pressure.
constexpr int TL_XB = 1024, TL_YB = 256;
__host__ __device__ inline size_t tl_extra_bytes(int n) {
  return sizeof(float) * NAG * NAG + sizeof(double) * ((WG / 64) * NAG + NAG) + (size_t)((n + 7) & ~7);
}
// The set-up of the two-level preconditioner (shared by cg_pressure_2l_lds and cg_pressure_2l_onchip): aggregates AG[n] by the
// histogram rule, coarse matrix by LDS atomics, its Gauss-Jordan inverse, the exactly symmetric fp32 copy AI [NAG][NAG].
// `hist`: LDS scratch of 4 (TL_XB + NAGX TL_YB + 2 NAGX) + n bytes; AC: LDS [NAG][NAG] doubles (may alias `hist`: the
// histograms are dead when it is zeroed); red: the reduction scratch ([32..63] used here).  Ends WITHOUT a barrier behind AI.
__device__ __forceinline__ void tl_build(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A, const double* coords,
                                         int* hist, double* AC, float* AI, unsigned char* AG, double* red) {
  constexpr int NW = WG / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- aggregates
  {
    int* HX = hist;                               // [TL_XB] counts, then exclusive prefix sums
    int* HY = HX + TL_XB;                         // [NAGX][TL_YB]
    int* SC = HY + NAGX * TL_YB;                  // [NAGX] population of a strip ([NW] wave totals of the scan behind it)
    unsigned char* ST = reinterpret_cast<unsigned char*>(SC + 2 * NAGX);   // [n] strip of a vertex
    double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
    for (int i = tid; i < n; i += WG) {
      const double cx = coords[2 * i], cy = coords[2 * i + 1];
      lo[0] = fmin(lo[0], cx);
      hi[0] = fmax(hi[0], cx);
      lo[1] = fmin(lo[1], cy);
      hi[1] = fmax(hi[1], cy);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
      for (int off = 32; off > 0; off >>= 1) {
        lo[c] = fmin(lo[c], __shfl_xor(lo[c], off));
        hi[c] = fmax(hi[c], __shfl_xor(hi[c], off));
      }
    if (lane == 0) {
      red[32 + wave] = lo[0];
      red[40 + wave] = hi[0];
      red[48 + wave] = lo[1];
      red[56 + wave] = hi[1];
    }
    for (int k = tid; k < TL_XB + NAGX * TL_YB + NAGX; k += WG) HX[k] = 0;
    __syncthreads();
#pragma unroll
    for (int w_ = 0; w_ < NW; ++w_) {
      lo[0] = fmin(lo[0], red[32 + w_]);
      hi[0] = fmax(hi[0], red[40 + w_]);
      lo[1] = fmin(lo[1], red[48 + w_]);
      hi[1] = fmax(hi[1], red[56 + w_]);
    }
    const double sx = hi[0] > lo[0] ? TL_XB / (hi[0] - lo[0]) : 0.0, sy = hi[1] > lo[1] ? TL_YB / (hi[1] - lo[1]) : 0.0;
    auto xbin = [&](int i) { return min(TL_XB - 1, (int)((coords[2 * i] - lo[0]) * sx)); };
    auto ybin = [&](int i) { return min(TL_YB - 1, (int)((coords[2 * i + 1] - lo[1]) * sy)); };
    for (int i = tid; i < n; i += WG) atomicAdd(&HX[xbin(i)], 1);
    __syncthreads();
    {  // exclusive prefix sums of the 1 024 counts: two bins per thread, scan over the workgroup
      const int c0 = HX[2 * tid], c1 = HX[2 * tid + 1];
      int s_ = c0 + c1;
      for (int off = 1; off < 64; off <<= 1) {
        const int t_ = __shfl_up(s_, off);
        if (lane >= off) s_ += t_;
      }
      int* WT = SC + NAGX;                        // [NW] wave totals
      if (lane == 63) WT[wave] = s_;
      __syncthreads();
      int before = 0;
      for (int w_ = 0; w_ < wave; ++w_) before += WT[w_];
      const int ex = before + s_ - c0 - c1;
      HX[2 * tid] = ex;
      HX[2 * tid + 1] = ex + c0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += WG) {
      const int st = min(NAGX - 1, (int)((long long)HX[xbin(i)] * NAGX / n));
      ST[i] = (unsigned char)st;
      atomicAdd(&SC[st], 1);
      atomicAdd(&HY[st * TL_YB + ybin(i)], 1);
    }
    __syncthreads();
    {  // per strip (= wave): exclusive prefix sums of its 256 counts, four bins per lane
      int* h = HY + wave * TL_YB + 4 * lane;
      const int c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
      int s_ = c0 + c1 + c2 + c3;
      for (int off = 1; off < 64; off <<= 1) {
        const int t_ = __shfl_up(s_, off);
        if (lane >= off) s_ += t_;
      }
      const int ex = s_ - (c0 + c1 + c2 + c3);
      h[0] = ex;
      h[1] = ex + c0;
      h[2] = ex + c0 + c1;
      h[3] = ex + c0 + c1 + c2;
    }
    __syncthreads();
    for (int i = tid; i < n; i += WG) {
      const int st = ST[i];
      const int cell = min(NAGY - 1, (int)((long long)HY[st * TL_YB + ybin(i)] * NAGY / max(SC[st], 1)));
      AG[i] = (unsigned char)(st * NAGY + cell);
    }
  }
  // ---- coarse matrix (fp64, in p | q), its inverse, the fp32 copy
  // (in LDS behind the tables when `extra` has the room - the instances with global vectors -, else in the scratch)
  __syncthreads();
  for (int e = tid; e < NAG * NAG; e += WG) AC[e] = 0.0;
  __syncthreads();
  {
    const int nsl = (n + 63) >> 6;
    for (int s_ = wave; s_ < nsl; s_ += NW) {
      const int base = sl_off[s_], wd = (sl_off[s_ + 1] - base) >> 6;
      const int row = (s_ << 6) + lane;
      if (row < n) {
        const int ar = AG[row] * NAG;
        for (int j = 0; j < wd; ++j) {
          const double av = A[base + lane + j * 64];
          if (av != 0.0) atomicAdd(&AC[ar + AG[sl_col[base + lane + j * 64]]], av);
        }
      }
    }
  }
  __syncthreads();
  if (tid < NAG && AC[tid * NAG + tid] == 0.0) AC[tid * NAG + tid] = 1.0;   // (an empty aggregate)
  __syncthreads();
  {
    constexpr int EPT = (NAG * NAG + WG - 1) / WG;
    int ei_[EPT], ej_[EPT];
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
      const int e = tid + m * WG;
      ei_[m] = e / NAG;
      ej_[m] = e - ei_[m] * NAG;
    }
    for (int kk = 0; kk < NAG; ++kk) {
      const double ip = 1.0 / AC[kk * NAG + kk];
      double nv_[EPT];
#pragma unroll
      for (int m = 0; m < EPT; ++m) {
        const int e = tid + m * WG;
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
        const int e = tid + m * WG;
        if (e < NAG * NAG) AC[e] = nv_[m];
      }
      __syncthreads();
    }
    // fp32 copy, exactly symmetric: the entry of the upper triangle for both (i, j) and (j, i)
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
      const int e = tid + m * WG;
      if (e < NAG * NAG) AI[e] = (float)AC[min(ei_[m], ej_[m]) * NAG + max(ei_[m], ej_[m])];
    }
  }
}

__device__ __attribute__((noinline)) int cg_pressure_2l_lds(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A, const double* coords,
                                         double rtol, int maxit, double* x, double* r, double* p, double* q,
                                         size_t scratch_bytes, double* extra, size_t extra_bytes, double* red) {
  constexpr int NW = WG / 64;
  static_assert(NW == NAGX, "one wave per strip in the y pass");
  static_assert(sizeof(float) * NAG * NAG % 8 == 0, "alignment of the partial restrictions");
  // (`scratch_bytes`: what is contiguous behind p - p | q in LDS, the slab vector of p in global memory)
  if (n < 4 * NAG || tl_extra_bytes(n) > extra_bytes || scratch_bytes < sizeof(double) * NAG * NAG ||
      scratch_bytes < sizeof(int) * (TL_XB + NAGX * TL_YB + 2 * NAGX) + (size_t)n)
    return -1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* AI = reinterpret_cast<float*>(extra);                             // [NAG][NAG] inverse of the coarse matrix
  double* WP = extra + NAG * NAG / 2;                                      // [NW][NAG] per-wave partial restrictions
  double* YV = WP + NW * NAG;                                              // [NAG] coarse result
  unsigned char* AG = reinterpret_cast<unsigned char*>(YV + NAG);          // [n] aggregate of a vertex
  double acc[2] = {0.0, 0.0};
  __syncthreads();
  spmv_sell(sl_off, sl_col, A, x, n, [&](int row, double y0) {
    const double b = r[row];
    const double r0 = b - y0;
    r[row] = r0;
    acc[0] += b * b;
    acc[1] += r0 * r0;
  });
  block_sum<2>(acc, red);
  const double bb = acc[0], tol2 = rtol * rtol * bb;
  double rr = acc[1];
  if (!(rr > tol2) || bb == 0.0) return 0;
  // ---- aggregates, coarse matrix (fp64: in LDS behind the tables when `extra` has the room - the instances with global
  //      vectors -, else in the scratch p | q), its inverse, the fp32 copy
  tl_build(n, sl_off, sl_col, A, coords, reinterpret_cast<int*>(p),
           extra_bytes >= tl_extra_bytes(n) + sizeof(double) * NAG * NAG
               ? reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(extra) + tl_extra_bytes(n)) : p,
           AI, AG, red);
  __syncthreads();
  int rsel = 0;
  double rz_old = 1.0;
  int it = 0;
  while (it < maxit) {
    // ---- z = r + P A_c^-1 P^T r
    if (lane < NAG) WP[wave * NAG + lane] = 0.0;
    for (int i = tid; i < n; i += WG) atomicAdd(&WP[wave * NAG + AG[i]], r[i]);
    __syncthreads();
    if (tid < NAG * 8) {
      const int I = tid >> 3, part = tid & 7;
      double s_ = 0.0;
      for (int J = part; J < NAG; J += 8) {
        double w_ = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < NW; ++w2) w_ += WP[w2 * NAG + J];
        s_ += (double)AI[I * NAG + J] * w_;
      }
      s_ += dpp_get<0xB1, 0xF>(s_);      // quad_perm [1,0,3,2]
      s_ += dpp_get<0x4E, 0xF>(s_);      // quad_perm [2,3,0,1]
      s_ += dpp_get<0x141, 0xF>(s_);     // row_half_mirror: the other quad of the group of 8
      if (part == 0) YV[I] = s_;
    }
    __syncthreads();
    double a0[1] = {0.0};
    for (int i = tid; i < n; i += WG) {
      const double ri = r[i], z = ri + YV[AG[i]];
      q[i] = z;
      a0[0] += ri * z;
    }
    block_sum1<1>(a0, red, rsel);
    const double rz = a0[0];
    const double beta = rz / rz_old;
    rz_old = rz;
    if (it == 0)
      for (int i = tid; i < n; i += WG) p[i] = q[i];
    else
      for (int i = tid; i < n; i += WG) p[i] = q[i] + beta * p[i];
    ++it;
    __syncthreads();
    double a1[1] = {0.0};
    spmv_sell(sl_off, sl_col, A, p, n, [&](int row, double y0) {
      q[row] = y0;
      a1[0] += p[row] * y0;
    });
    block_sum1<1>(a1, red, rsel);
    if (!(a1[0] > 0.0)) break;
    const double alpha = rz / a1[0];
    double a2[1] = {0.0};
    for (int i = tid; i < n; i += WG) {
      x[i] += alpha * p[i];
      const double rn = r[i] - alpha * q[i];
      r[i] = rn;
      a2[0] += rn * rn;
    }
    block_sum1<1>(a2, red, rsel);
    rr = a2[0];
    if (!(rr > tol2)) break;
  }
  __syncthreads();
  return it;
}

// ------------------------------------------------------------------ two-level PCG with the MATRIX ON THE CHIP (round 6)
//
// cg_pressure_2l_lds keeps the four CG vectors in LDS and streams the matrix from L2 in every iteration: on the red-refined
// ys930 (3 322 rows, 25.5 k SELL entries = 300 KB) an iteration lasts 16.4 us, i.e. 18 GB/s - what ONE workgroup pulls out
// of L2 (HISTORY 8.5) - and the 171 iterations of a fresh mesh are 2.8 ms of the S3 step's flow leg.  Here the matrix does
// not move after the set-up: thread t owns rows t + k WG (k < K <= 7) = lane t % 64 of SELL slice 8 k + t / 64, so the slices
// of the first OC_KR row groups are held in REGISTERS by their owner (OC_WR entries per row: fp64 value + 16-bit column,
// padded with zero values) and the remaining slices are copied to LDS (fp64 values + 16-bit columns, the SELL layout as it
// is); x, r, q, z of the own rows live in registers, only the search direction p - the one vector that is gathered - in LDS,
// and the fp32 inverse of the coarse matrix in registers of the 448 threads of the coarse product.  An iteration is then
// LDS gathers + five workgroup barriers.  Same preconditioner (tl_build), same recurrences, same stopping test as
// cg_pressure_2l_lds; the row sums run over the SELL columns in the same order.  U: the kernel's LDS union; in: U[0..n) = x0,
// U[NVp..NVp+n) = b; out: U[0..n) = x.  Returns the iterations, or -1 WITHOUT having touched anything when the mesh does
// not fit (more than 7 row groups, a register slice wider than OC_WR, the LDS slices beyond U).
constexpr int OC_KR = 4, OC_WR = 10, OC_KMAX = 7;
__device__ __attribute__((noinline)) int cg_pressure_2l_onchip(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A,
                                                                const double* coords, double rtol, int maxit, double* U, size_t U_bytes,
                                                                int NVp, double* red) {
  constexpr int NW = WG / 64;
  static_assert(NW == NAGX && NAG * 8 <= WG && OC_WR % 2 == 0, "one wave per strip; 8 threads per coarse row");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nsl = (n + 63) >> 6, K = (nsl + NW - 1) / NW;
  if (n < 4 * NAG || K > OC_KMAX || n > 0xFFFF) return -1;
  // ---- LDS plan: p [NP] | WP [NW][NAG] | YV [NAG] | AG [n] | LDS slices: values, then columns
  const int NP = (n + 7) & ~7;
  const int s_l0 = min(OC_KR * NW, nsl);                       // first slice that lives in LDS
  const int e_l0 = sl_off[s_l0], ent_l = sl_off[nsl] - e_l0;   // its first entry; entries in LDS
  double* P = U;
  double* WP = P + NP;
  double* YV = WP + NW * NAG;
  unsigned char* AG = reinterpret_cast<unsigned char*>(YV + NAG);
  double* LV = reinterpret_cast<double*>(AG + NP);
  unsigned short* LC = reinterpret_cast<unsigned short*>(LV + ent_l);
  const size_t need = sizeof(double) * (size_t)(NP + NW * NAG + NAG + ent_l) + (size_t)NP + sizeof(unsigned short) * (size_t)(ent_l + 8);
  // (the set-up's scratch - histograms, the fp64 coarse matrix, its fp32 inverse - lies where the LDS slices go afterwards)
  const size_t setup = sizeof(double) * (size_t)(NP + NW * NAG + NAG) + (size_t)NP + sizeof(double) * NAG * NAG + sizeof(float) * NAG * NAG +
                       sizeof(int) * (TL_XB + NAGX * TL_YB + 2 * NAGX) + (size_t)NP;
  bool bad = need > U_bytes || setup > U_bytes;
#pragma unroll
  for (int k = 0; k < OC_KR; ++k) {
    const int s_ = k * NW + wave;
    if (s_ < nsl && ((sl_off[s_ + 1] - sl_off[s_]) >> 6) > OC_WR) bad = true;
  }
  if (__syncthreads_or(bad)) return -1;
  // ---- own rows of x0 and b
  double x[OC_KMAX], r[OC_KMAX], q[OC_KMAX];
#pragma unroll
  for (int k = 0; k < OC_KMAX; ++k) {
    const int row = tid + k * WG;
    x[k] = row < n ? U[row] : 0.0;
    r[k] = row < n ? U[NVp + row] : 0.0;
  }
  int lb[OC_KMAX - OC_KR], lw[OC_KMAX - OC_KR];                 // LDS slices of this wave: first entry (relative), width
#pragma unroll
  for (int k = OC_KR; k < OC_KMAX; ++k) {
    const int s_ = k * NW + wave;
    lb[k - OC_KR] = __builtin_amdgcn_readfirstlane(s_ < nsl ? sl_off[s_] - e_l0 : 0);
    lw[k - OC_KR] = __builtin_amdgcn_readfirstlane(s_ < nsl ? (sl_off[s_ + 1] - sl_off[s_]) >> 6 : 0);
  }
  __syncthreads();                                              // (b is in registers: its LDS is free from here on)
  // ---- the preconditioner (scratch where the LDS slices go), its fp32 inverse into registers
  float ai[(NAG + 7) / 8];
  {
    double* AC = LV;
    float* AI = reinterpret_cast<float*>(AC + NAG * NAG);
    int* hist = reinterpret_cast<int*>(AI + NAG * NAG);
    tl_build(n, sl_off, sl_col, A, coords, hist, AC, AI, AG, red);
    __syncthreads();
    const int I = tid >> 3, part = tid & 7;
#pragma unroll
    for (int m = 0; m < (NAG + 7) / 8; ++m) ai[m] = (tid < NAG * 8 && part + 8 * m < NAG) ? AI[I * NAG + part + 8 * m] : 0.0f;
  }
  unsigned agp[2] = {0u, 0u};                                   // aggregates of the own rows, one byte each
#pragma unroll
  for (int k = 0; k < OC_KMAX; ++k) agp[k >> 2] |= (tid + k * WG < n ? (unsigned)AG[tid + k * WG] : 0u) << (8 * (k & 3));
  auto ag = [&](int k) { return (int)((agp[k >> 2] >> (8 * (k & 3))) & 0xFFu); };
  __syncthreads();
  // ---- the LDS slices
  for (int e = tid; e < ent_l; e += WG) {
    LV[e] = A[e_l0 + e];
    LC[e] = (unsigned short)sl_col[e_l0 + e];
  }
  __syncthreads();
  // (the register slices are loaded LAST: across the set-up above they were the allocator's first spill candidates)
  double av[OC_KR][OC_WR];
  unsigned ac[OC_KR][OC_WR / 2];
#pragma unroll
  for (int k = 0; k < OC_KR; ++k) {
    const int s_ = k * NW + wave, own = min(tid + k * WG, n - 1);
    const int base = s_ < nsl ? sl_off[s_] : 0, wd = s_ < nsl ? (sl_off[s_ + 1] - base) >> 6 : 0;
#pragma unroll
    for (int j = 0; j < OC_WR; j += 2) {
      const bool h0 = j < wd, h1 = j + 1 < wd;
      av[k][j] = h0 ? A[base + lane + j * 64] : 0.0;
      av[k][j + 1] = h1 ? A[base + lane + (j + 1) * 64] : 0.0;
      const unsigned c0 = h0 ? (unsigned)sl_col[base + lane + j * 64] : (unsigned)own;
      const unsigned c1 = h1 ? (unsigned)sl_col[base + lane + (j + 1) * 64] : (unsigned)own;
      ac[k][j / 2] = c0 | (c1 << 16);
    }
  }
  auto spmv = [&](double (&y)[OC_KMAX]) {
#pragma unroll
    for (int k = 0; k < OC_KR; ++k) {
      double s_ = 0.0;
#pragma unroll
      for (int j = 0; j < OC_WR; j += 2) {
        // (opaque: the 40 gather addresses are loop invariants the compiler would otherwise keep in 40 registers - and spill)
        asm volatile("" : "+v"(ac[k][j / 2]));
        const unsigned c = ac[k][j / 2];
        s_ += av[k][j] * P[c & 0xFFFFu];
        s_ += av[k][j + 1] * P[c >> 16];
      }
      y[k] = s_;
      __builtin_amdgcn_sched_barrier(0);       // (row by row: all 40 gathers in flight at once cost 80 registers and spilled)
    }
#pragma unroll
    for (int k = OC_KR; k < OC_KMAX; ++k) {
      double s_ = 0.0;
      const double* a = LV + lb[k - OC_KR] + lane;
      const unsigned short* c = LC + lb[k - OC_KR] + lane;
      for (int j = 0; j < lw[k - OC_KR]; ++j) s_ += a[j * 64] * P[c[j * 64]];
      y[k] = s_;
    }
  };
  // ---- r = b - A x0
  double acc[2] = {0.0, 0.0};
  spmv(q);
#pragma unroll
  for (int k = 0; k < OC_KMAX; ++k)
    if (tid + k * WG < n) {
      const double b = r[k], r0 = b - q[k];
      r[k] = r0;
      acc[0] += b * b;
      acc[1] += r0 * r0;
    }
  block_sum<2>(acc, red);
  const double bb = acc[0], tol2 = rtol * rtol * bb;
  double rr = acc[1];
  int it = 0;
  if (rr > tol2 && bb != 0.0) {
    int rsel = 0;
    double rz_old = 1.0;
    while (it < maxit) {
      // z = r + P A_c^-1 P^T r
      if (lane < NAG) WP[wave * NAG + lane] = 0.0;
#pragma unroll
      for (int k = 0; k < OC_KMAX; ++k)
        if (tid + k * WG < n) atomicAdd(&WP[wave * NAG + ag(k)], r[k]);
      __syncthreads();
      if (tid < NAG * 8) {
        const int I = tid >> 3, part = tid & 7;
        int part_o = part;
        asm volatile("" : "+v"(part_o));            // (one base address + immediate offsets instead of 56 hoisted addresses)
        const double* wq = WP + part_o;
        double s_ = 0.0;
        static_assert(NAG % 8 == 0, "every thread of a coarse row has NAG / 8 columns");
#pragma unroll
        for (int m = 0; m < NAG / 8; ++m) {
          double w_ = 0.0;
#pragma unroll
          for (int w2 = 0; w2 < NW; ++w2) w_ += wq[w2 * NAG + 8 * m];
          s_ += (double)ai[m] * w_;
        }
        s_ += dpp_get<0xB1, 0xF>(s_);      // quad_perm [1,0,3,2]
        s_ += dpp_get<0x4E, 0xF>(s_);      // quad_perm [2,3,0,1]
        s_ += dpp_get<0x141, 0xF>(s_);     // row_half_mirror: the other quad of the group of 8
        if (part == 0) YV[I] = s_;
      }
      __syncthreads();
      double a0[1] = {0.0};
#pragma unroll
      for (int k = 0; k < OC_KMAX; ++k)
        if (tid + k * WG < n) a0[0] += r[k] * (r[k] + YV[ag(k)]);
      block_sum1<1>(a0, red, rsel);
      const double rz = a0[0];
      const double beta = rz / rz_old;
      rz_old = rz;
#pragma unroll
      for (int k = 0; k < OC_KMAX; ++k)
        if (tid + k * WG < n) {
          const double z = r[k] + YV[ag(k)];          // (read again instead of kept across the reduction: 14 registers)
          P[tid + k * WG] = it == 0 ? z : z + beta * P[tid + k * WG];
        }
      ++it;
      __syncthreads();
      double a1[1] = {0.0};
      spmv(q);
#pragma unroll
      for (int k = 0; k < OC_KMAX; ++k)
        if (tid + k * WG < n) a1[0] += P[tid + k * WG] * q[k];
      block_sum1<1>(a1, red, rsel);
      if (!(a1[0] > 0.0)) break;
      const double alpha = rz / a1[0];
      double a2[1] = {0.0};
#pragma unroll
      for (int k = 0; k < OC_KMAX; ++k)
        if (tid + k * WG < n) {
          x[k] += alpha * P[tid + k * WG];
          const double rn = r[k] - alpha * q[k];
          r[k] = rn;
          a2[0] += rn * rn;
        }
      block_sum1<1>(a2, red, rsel);
      rr = a2[0];
      if (!(rr > tol2)) break;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < OC_KMAX; ++k)
    if (tid + k * WG < n) U[tid + k * WG] = x[k];
  __syncthreads();
  return it;
}

// the Krylov pressure solve of the kernels whose pressure vectors live in LDS (modes 0 / 4 / 5 / 7): two-level from
// TL_AUTO_NV vertices on (pcg_degree 0 = auto) or on request (pcg_degree < 0), Jacobi-CG otherwise (pcg_degree > 0: always)
#ifndef MDQ_TL_AUTO_NV
#define MDQ_TL_AUTO_NV 2048
#endif
__device__ inline int pressure_krylov_lds(const mdq_ipcs_desc& d, bool k1_lds, int n, const int32_t* sl_off, const int32_t* sl_col,
                                          const double* A, const double* coords, double* x, double* r, double* p, double* q,
                                          size_t scratch_bytes, double* extra, size_t extra_bytes, double* red,
                                          double* U = nullptr, size_t U_bytes = 0, int NVp = 0) {
  int it = -1;
  // (U: the LDS union of the kernel with x = U, r = U + NVp: the matrix-on-chip solver where the mesh fits it; pcg_degree -2
  //  keeps round 5's solver with the matrix streamed from L2 - A / B switch)
  if (!k1_lds && U != nullptr && d.pcg_degree != -2 && (d.pcg_degree < 0 || (d.pcg_degree == 0 && n >= MDQ_TL_AUTO_NV)))
    it = cg_pressure_2l_onchip(n, sl_off, sl_col, A, coords, d.rtol, d.maxit_p, U, U_bytes, NVp, red);
  if (it < 0 && !k1_lds && (d.pcg_degree < 0 || (d.pcg_degree == 0 && n >= MDQ_TL_AUTO_NV)))
    it = cg_pressure_2l_lds(n, sl_off, sl_col, A, coords, d.rtol, d.maxit_p, x, r, p, q, scratch_bytes, extra, extra_bytes, red);
  if (it < 0) it = cg_pressure(n, sl_off, sl_col, A, d.rtol, d.maxit_p, x, r, p, q, red);
  return it;
}

#ifdef MDQ_AT_TRACE
// debug build only: s_memtime deltas of thread 0 of environment 0 at the phase boundaries of at_velocity_kernel
static __device__ long long mdq_at_trace_buf[16];
#define AT_STAMP(k) { const long long tn_ = __builtin_amdgcn_s_memtime(); if (tid == 0 && b == 0) mdq_at_trace_buf[k] += tn_ - tq_; tq_ = tn_; }
static __device__ long long mdq_pt_trace_buf[16];
#define PT_STAMP(k) { const long long tn_ = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0 && blockIdx.x == 0) mdq_pt_trace_buf[k] += tn_ - tqp_; tqp_ = tn_; }
static __device__ long long mdq_ct_trace_buf[16];
#define CT_STAMP(k) { const long long tn_ = __builtin_amdgcn_s_memtime(); if (tid == 0 && b == 0) mdq_ct_trace_buf[k] += tn_ - tq_; tq_ = tn_; }
#else
#define AT_STAMP(k)
#define CT_STAMP(k)
#define PT_STAMP(k)
#endif

// ================================================================== direct pressure solve
//
// Solve phase of the substructuring factorisation built by meshdqn_amd/pressure_direct.py
// (the MI355X counterpart of the MUMPS back-substitution of flow_solver.py:380): dense
// column-major blocks, one thread per row, coalesced streaming, three barriers per solve.
struct PdView {
  int nI, nG, nparts;
  const int32_t *node, *meta, *rowblk, *gidx, *gk_ptr, *gk_col;
  const double *W, *F, *Sinv, *gk_val;
};

__device__ __forceinline__ PdView pd_view(const mdq_ipcs_desc& d, int b) {
  PdView p;
  const int64_t B = b;
  const int32_t* h = d.pd_hdr + B * 4;
  p.nI = h[0];
  p.nG = h[1];
  p.nparts = h[2];
  p.node = d.pd_node + B * d.NV;
  p.meta = d.pd_meta + B * d.NPART * 6;
  p.rowblk = d.pd_rowblk + B * d.NV;
  p.W = d.pd_W + B * d.NPW;
  p.F = d.pd_F + B * d.NPF;
  p.gidx = d.pd_gidx + B * d.NPGI;
  p.Sinv = d.pd_Sinv + B * d.NPS;
  p.gk_ptr = d.pd_gk_ptr + B * (d.NV + 1);
  p.gk_col = d.pd_gk_col + B * d.NPGK;
  p.gk_val = d.pd_gk_val + B * d.NPGK;
  return p;
}

// sum_j A[j * stride] * x[idx(j)], j in [0, len): the strided global loads in batches of PDU, ALL of a batch in flight
// together; the last batch is padded with clamped (re-read, weight 0) entries, so there is no serial remainder loop
// (with `#pragma unroll 8/16` the remainder of a 55-column block is up to 15 dependent round trips to the memory side).
constexpr int PDU = 16;
template <class Idx>
__device__ __forceinline__ double pd_dot(const double* __restrict__ A, int64_t stride, int len, const double* x, Idx idx) {
  double acc = 0.0;
  for (int j0 = 0; j0 < len; j0 += PDU) {
    double av[PDU];
    int xi[PDU];
#pragma unroll
    for (int u = 0; u < PDU; ++u) {
      const int j = min(j0 + u, len - 1);
      av[u] = A[(int64_t)j * stride];
      xi[u] = idx(j);
    }
#pragma unroll
    for (int u = 0; u < PDU; ++u) acc += (j0 + u < len ? av[u] : 0.0) * x[xi[u]];
  }
  return acc;
}

// x = K^-1 b.  b, x: LDS vectors in natural node order (x may alias b); t0,t1,t2: LDS scratch
// of at least max(n, NTH) doubles each (NTH = threads of the calling kernel).
template <int NTH = WG>
__device__ inline void pressure_direct(const PdView& pd, int n, const double* b, double* x, double* t0, double* t1,
                                       double* t2) {
  const int tid = threadIdx.x, nI = pd.nI, nG = pd.nG;
  double* bp = t0;  // permuted right-hand side
  double* y = t1;   // W b_I  |  separator: g, then x_G
#ifdef MDQ_AT_TRACE
  long long tqp_ = __builtin_amdgcn_s_memtime();
#endif
  __syncthreads();
  for (int q = tid; q < n; q += NTH) bp[q] = b[pd.node[q]];
  __syncthreads();
  PT_STAMP(1)
  // y_I = W b_I
  for (int q = tid; q < nI; q += NTH) {
    const int32_t* m6 = pd.meta + 6 * pd.rowblk[q];
    const int q0 = m6[0], m = m6[1];
    const double* Wc = pd.W + m6[2] + (q - q0);
    y[q] = pd_dot(Wc, m, m, bp, [&](int j) { return q0 + j; });
  }
  __syncthreads();
  PT_STAMP(2)
  // g = b_G - K[G,I] y_I
  for (int g = tid; g < nG; g += NTH) {
    double acc = bp[nI + g];
    for (int k = pd.gk_ptr[g]; k < pd.gk_ptr[g + 1]; ++k) acc -= pd.gk_val[k] * y[pd.gk_col[k]];
    y[nI + g] = acc;
  }
  __syncthreads();
  PT_STAMP(3)
  // x_G = Sinv g : rows split over column slices so that all waves stream Sinv
  const int NGP = (nG + 63) & ~63;
  const int nsl = NGP > 0 ? (NTH / NGP > 0 ? NTH / NGP : 1) : 1;
  const int cw = (nG + nsl - 1) / nsl;
  for (int idx = tid; idx < nsl * NGP; idx += NTH) {
    const int sl = idx / NGP, row = idx - sl * NGP;
    double acc = 0.0;
    if (row < nG) {
      const int c1 = min(nG, (sl + 1) * cw);
      const double* Sc = pd.Sinv + row;
#pragma unroll 8
      for (int c = sl * cw; c < c1; ++c) acc += Sc[(int64_t)c * nG] * y[nI + c];   // (pd_dot was slower here: 13 columns)
    }
    t2[idx] = acc;
  }
  __syncthreads();
  for (int g = tid; g < nG; g += NTH) {
    double acc = 0.0;
    for (int sl = 0; sl < nsl; ++sl) acc += t2[sl * NGP + g];
    bp[g] = acc;  // x_G (bp is free now)
  }
  __syncthreads();
  PT_STAMP(4)
  // x_I = y_I - F x_G ; scatter back to natural order
  for (int q = tid; q < nI; q += NTH) {
    const int32_t* m6 = pd.meta + 6 * pd.rowblk[q];
    const int q0 = m6[0], m = m6[1], gs = m6[4];
    const double* Fc = pd.F + m6[3] + (q - q0);
    const int32_t* gi = pd.gidx + m6[5];
    double acc = y[q];
    if (gs > 0) acc -= pd_dot(Fc, m, gs, bp, [&](int c) { return gi[c]; });
    x[pd.node[q]] = acc;
  }
  for (int g = tid; g < nG; g += NTH) x[pd.node[nI + g]] = bp[g];
  __syncthreads();
  PT_STAMP(5)
}

}  // namespace mdq
