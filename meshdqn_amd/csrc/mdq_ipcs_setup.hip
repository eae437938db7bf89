// IPCS: assembly of the SELL operators (assemble_kernel) and the matrix-free operator set-up (setup_matfree_kernel).
// Included by mdq_ipcs.hip (the entry unit) only, behind the per-environment views.
namespace mdq {

// ================================================================== assembly

// B^{cd}_e[i][j] = int_{outflow facet k of cell e} phi_i (d_c phi_j) n_d ds
// (`- dot(mu*nabla_grad(U)*n, v)*ds`, flow_solver.py:109), 2-point Gauss (degree 3 integrand).
__device__ inline void outflow_entry(const EnvView& v, int e, int k, int i, int j, const Geo& g, double (&Bcd)[2][2]) {
  double X[3][2];
  load_cell_coords(v, e, X);
  const Facet f = facet_geometry(X, k);
  Bcd[0][0] = Bcd[0][1] = Bcd[1][0] = Bcd[1][1] = 0.0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double s = c_tab.gx[q], w = c_tab.gw[q] * f.len;
    const double xi = f.ra[0] + s * (f.rb[0] - f.ra[0]);
    const double eta = f.ra[1] + s * (f.rb[1] - f.ra[1]);
    const double l0 = 1.0 - xi - eta;
    const double phi = p2_phi_one(i, l0, xi, eta);
    double dx, dy;
    p2_dphi_one(j, l0, xi, eta, dx, dy);
    const double gxp = g.j00 * dx + g.j10 * dy;  // physical d/dx phi_j
    const double gyp = g.j01 * dx + g.j11 * dy;
    Bcd[0][0] += w * phi * gxp * f.nx;
    Bcd[0][1] += w * phi * gxp * f.ny;
    Bcd[1][0] += w * phi * gyp * f.nx;
    Bcd[1][1] += w * phi * gyp * f.ny;
  }
}

static __global__ __launch_bounds__(WG) void assemble_kernel(mdq_ipcs_desc d) {
  const int b = blockIdx.x;
  EnvView v = env_view(d, b);
  v.nnz2 = v.rowptr2[v.n2];
  v.nnz1 = v.rowptr1[v.nv];
  const int tid = threadIdx.x;
  const double a = v.rho / v.dt, mu = v.mu;

  // ---- phase 0: affine geometry per triangle
  for (int e = tid; e < v.nt; e += WG) {
    double X[3][2];
    load_cell_coords(v, e, X);
    const double J00 = X[1][0] - X[0][0], J01 = X[2][0] - X[0][0];
    const double J10 = X[1][1] - X[0][1], J11 = X[2][1] - X[0][1];
    const double det = J00 * J11 - J01 * J10;
    v.geom[0 * v.NT + e] = J11 / det;
    v.geom[1 * v.NT + e] = -J01 / det;
    v.geom[2 * v.NT + e] = -J10 / det;
    v.geom[3 * v.NT + e] = J00 / det;
    v.geom[4 * v.NT + e] = fabs(det);
  }
  __syncthreads();

  // position of entry j of row r inside the SELL-64 arrays
  auto pos2 = [&](int r, int j) { return v.sl2_off[r >> 6] + j * 64 + (r & 63); };
  auto pos1 = [&](int r, int j) { return v.sl1_off[r >> 6] + j * 64 + (r & 63); };

  // ---- phase 1: full (pre-BC) operator values, one thread per non-zero
  for (int k = tid; k < v.nnz2; k += WG) {
    double m = 0.0, kxx = 0.0, kxy = 0.0, kyx = 0.0, kyy = 0.0;
    double bxx = 0.0, bxy = 0.0, byx = 0.0, byy = 0.0;
    const int s0 = v.asm2_ptr[k], s1 = v.asm2_ptr[k + 1];
    int row = 0;
    for (int s = s0; s < s1; ++s) {
      const int slot = v.asm2_src[s];
      const int e = slot / 36, ij = slot - e * 36, i = ij / 6, j = ij - i * 6;
      if (s == s0) row = v.cell_dofs[i * v.NT + e];
      const Geo g = load_geo(v, e);
      m += g.det * c_tab.Mhat[i][j];
      // K^{ab}_ij = det * sum_{cd} Jinv[c][a] Jinv[d][b] Ghat[c][d][i][j]
      const double g00 = c_tab.Ghat[0][0][i][j], g01 = c_tab.Ghat[0][1][i][j];
      const double g10 = c_tab.Ghat[1][0][i][j], g11 = c_tab.Ghat[1][1][i][j];
      // Jinv[c][a]: c = reference index (row), a = physical index (col)
      const double Ja[2][2] = {{g.j00, g.j01}, {g.j10, g.j11}};
      kxx += g.det * (Ja[0][0] * (Ja[0][0] * g00 + Ja[1][0] * g01) + Ja[1][0] * (Ja[0][0] * g10 + Ja[1][0] * g11));
      kxy += g.det * (Ja[0][0] * (Ja[0][1] * g00 + Ja[1][1] * g01) + Ja[1][0] * (Ja[0][1] * g10 + Ja[1][1] * g11));
      kyx += g.det * (Ja[0][1] * (Ja[0][0] * g00 + Ja[1][0] * g01) + Ja[1][1] * (Ja[0][0] * g10 + Ja[1][0] * g11));
      kyy += g.det * (Ja[0][1] * (Ja[0][1] * g00 + Ja[1][1] * g01) + Ja[1][1] * (Ja[0][1] * g10 + Ja[1][1] * g11));
      const int ko = v.cell_outflow[e];
      if (ko >= 0) {
        double Bcd[2][2];
        outflow_entry(v, e, ko, i, j, g, Bcd);
        bxx += Bcd[0][0];
        bxy += Bcd[0][1];
        byx += Bcd[1][0];
        byy += Bcd[1][1];
      }
    }
    const double L = kxx + kyy;
    // block(c,d) = a M delta_cd + mu/2 (delta_cd L + K^{dc}) - mu/2 B^{cd}
    double4 blk;
    blk.x = a * m + 0.5 * mu * (L + kxx) - 0.5 * mu * bxx;
    blk.y = 0.5 * mu * kyx - 0.5 * mu * bxy;
    blk.z = 0.5 * mu * kxy - 0.5 * mu * byx;
    blk.w = a * m + 0.5 * mu * (L + kyy) - 0.5 * mu * byy;
    const int ps = pos2(row, k - v.rowptr2[row]);
    reinterpret_cast<double4*>(v.A1)[ps] = blk;
    v.Ms[ps] = m;
  }
  for (int k = tid; k < v.nnz1; k += WG) {
    double kk = 0.0;
    const int s0 = v.asm1_ptr[k], s1 = v.asm1_ptr[k + 1];
    int row = 0;
    for (int s = s0; s < s1; ++s) {
      const int slot = v.asm1_src[s];
      const int e = slot / 9, ij = slot - e * 9, i = ij / 3, j = ij - i * 3;
      if (s == s0) row = v.cell_dofs[i * v.NT + e];
      const Geo g = load_geo(v, e);
      // grad lambda_i = Jinv^T dl_i, dl = (-1,-1),(1,0),(0,1)
      const double dix = sel3(i, -g.j00 - g.j10, g.j00, g.j10), diy = sel3(i, -g.j01 - g.j11, g.j01, g.j11);
      const double djx = sel3(j, -g.j00 - g.j10, g.j00, g.j10), djy = sel3(j, -g.j01 - g.j11, g.j01, g.j11);
      kk += 0.5 * g.det * (dix * djx + diy * djy);
    }
    v.K1s[pos1(row, k - v.rowptr1[row])] = kk;
  }
  // outflow row list of the matrix-free mode 3 (same facet integrals as above, kept separate)
  if (v.nbo > 0) {
    const int nbe = v.bo_ptr[v.nbo];
    for (int t = tid; t < nbe; t += WG) {
      const int slot = v.bo_src[t];
      const int e = slot / 36, ij = slot - e * 36, i = ij / 6, j = ij - i * 6;
      const Geo g = load_geo(v, e);
      double Bcd[2][2];
      outflow_entry(v, e, v.cell_outflow[e], i, j, g, Bcd);
      reinterpret_cast<double4*>(v.bo_val)[t] = make_double4(Bcd[0][0], Bcd[0][1], Bcd[1][0], Bcd[1][1]);
    }
  }
  __syncthreads();

  // ---- phase 2: Dirichlet lifting vectors and diagonals, one thread per row
  for (int r = tid; r < v.n2; r += WG) {
    double l1x = 0.0, l1y = 0.0, l3x = 0.0, dx = 1.0, dy = 1.0, dm = 1.0;
    const bool fr = v.bcu_flag[r] != 0;
    const int k0 = v.rowptr2[r], len = v.rowptr2[r + 1] - k0;
    for (int j = 0; j < len; ++j) {
      const int c = v.colidx2[k0 + j], ps = pos2(r, j);
      const double4 blk = reinterpret_cast<const double4*>(v.A1)[ps];
      if (v.bcu_flag[c]) {
        const double gx = v.bcu_gx[c];  // gy = 0 for every BC of the reference
        l1x += blk.x * gx;
        l1y += blk.z * gx;
        l3x += v.Ms[ps] * gx;
      }
      if (c == r && !fr) {
        dx = blk.x;
        dy = blk.w;
        dm = v.Ms[ps];
      }
    }
    v.lift1[r] = make_double2(l1x, l1y);
    v.lift3[r] = make_double2(l3x, 0.0);
    v.idiag1[r] = make_double2(1.0 / dx, 1.0 / dy);
    v.sdiagM[r] = sqrt(dm);
  }
  for (int r = tid; r < v.nv; r += WG) {
    double dk = 1.0;
    if (!v.bcp_flag[r]) {
      const int k0 = v.rowptr1[r], len = v.rowptr1[r + 1] - k0;
      for (int j = 0; j < len; ++j)
        if (v.colidx1[k0 + j] == r) dk = v.K1s[pos1(r, j)];
    }
    v.sdiagK[r] = sqrt(dk);
  }
  __syncthreads();

  // ---- phase 3: symmetric elimination + Jacobi scaling (+ zero the SELL padding)
  const int rows2 = ((v.n2 + 63) >> 6) << 6;
  for (int r = tid; r < rows2; r += WG) {
    const int width = (v.sl2_off[(r >> 6) + 1] - v.sl2_off[r >> 6]) >> 6;
    int len = 0;
    if (r < v.n2) {
      const bool fr = v.bcu_flag[r] != 0;
      const double2 id = v.idiag1[r];
      const double sr = v.sdiagM[r];
      const int k0 = v.rowptr2[r];
      len = v.rowptr2[r + 1] - k0;
      for (int j = 0; j < len; ++j) {
        const int c = v.colidx2[k0 + j], ps = pos2(r, j);
        const bool fc = v.bcu_flag[c] != 0;
        double4 blk = reinterpret_cast<const double4*>(v.A1)[ps];
        double m = v.Ms[ps];
        if (fr || fc) {
          const double one = (c == r) ? 1.0 : 0.0;
          blk = make_double4(one, 0.0, 0.0, one);
          m = one;
        } else {
          blk.x *= id.x;
          blk.y *= id.x;
          blk.z *= id.y;
          blk.w *= id.y;
          m = m / (sr * v.sdiagM[c]);
        }
        reinterpret_cast<double4*>(v.A1)[ps] = blk;
        v.Ms[ps] = m;
      }
    }
    for (int j = len; j < width; ++j) {
      const int ps = pos2(r, j);
      reinterpret_cast<double4*>(v.A1)[ps] = make_double4(0.0, 0.0, 0.0, 0.0);
      v.Ms[ps] = 0.0;
    }
  }
  const int rows1 = ((v.nv + 63) >> 6) << 6;
  for (int r = tid; r < rows1; r += WG) {
    const int width = (v.sl1_off[(r >> 6) + 1] - v.sl1_off[r >> 6]) >> 6;
    int len = 0;
    if (r < v.nv) {
      const bool fr = v.bcp_flag[r] != 0;
      const double sr = v.sdiagK[r];
      const int k0 = v.rowptr1[r];
      len = v.rowptr1[r + 1] - k0;
      for (int j = 0; j < len; ++j) {
        const int c = v.colidx1[k0 + j], ps = pos1(r, j);
        const bool fc = v.bcp_flag[c] != 0;
        double kk = v.K1s[ps];
        if (fr || fc)
          kk = (c == r) ? 1.0 : 0.0;
        else
          kk = kk / (sr * v.sdiagK[c]);
        v.K1s[ps] = kk;
      }
    }
    for (int j = len; j < width; ++j) v.K1s[pos1(r, j)] = 0.0;
  }
}

// ================================================================== matrix-free operator setup
//
// Everything mode 3 (with the CG pressure solver) needs from a NEW mesh, without any global sparsity pattern:
// geometry, outflow-row blocks, Jacobi diagonals and Dirichlet lifting vectors of A1 / M accumulated row-wise from
// the element matrices (dof <- element-slot gathers g2/g1), the scaled + BC-eliminated P1 Laplacian in SELL-64.
// Same numbers as assemble_kernel up to the summation order.  One workgroup per environment.
#ifdef MDQ_SETUP_TRACE
static __device__ long long mdq_st_trace_buf[16];
#define ST_STAMP(k) { __syncthreads(); const long long tn_ = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0 && blockIdx.x == 0) mdq_st_trace_buf[k] += tn_ - tq_; tq_ = tn_; }
extern "C" MDQ_API int mdq_st_trace_host(long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mdq_st_trace_buf), sizeof(long long) * 16) != hipSuccess) return -1;
  if (reset) { long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(mdq_st_trace_buf), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
#else
#define ST_STAMP(k)
#endif

// ST: the per-cell / per-dof data the row loops chase (geometry, cell dofs, Dirichlet flags and values, the P1 scaling) is
// staged in LDS first.  The row loops are chains of dependent loads (slot -> geometry / dofs -> flags -> values, per
// incident cell of every row): from global memory each level is an L2 round trip and the kernel was 270 k cycles of
// latency (P2 rows 134 k, P1 values 71 k, P1 diagonal 33 k); from LDS a level costs a tenth of that.
// 52 NT + 9 N2 + 9 NV bytes: 119 KB for ys930; a mesh that does not fit runs the unstaged instance.
constexpr int SWG = MDQ_SETUP_WG;   // threads of the set-up kernel (its row loops are latency chains: more rows in flight)
// LS (with ST): the dof <- element-slot lists (g1 / g2 pointers and slots, 16-bit in LDS) are staged as well when they fit:
// the row loops then have no dependent global load left.
// GEO = false with ST (round 6, the meshes whose 40 B of geometry per cell do not fit: the red-refined lab meshes): only the
// INDEX data is staged - cell dofs (16-bit), Dirichlet flags, the P1 scaling - 12 NT + N2 + 9 NV bytes (118 KB for the refined
// ys930); geometry and Dirichlet values come from global memory.  Of a slot's chain slot -> cell dofs -> flags (-> values at
// boundary cells only) the two inner levels are LDS round trips then; the unstaged instance paid an L2 round trip for each.
template <bool ST, bool LS = false, bool GEO = ST>
__global__ __launch_bounds__(SWG) void setup_matfree_kernel(mdq_ipcs_desc d) {
  static_assert(ST || !GEO, "geometry is staged together with the index data only");
  static_assert(GEO || !LS, "the slot lists are staged in the full instance only");
  const int b = blockIdx.x, tid = threadIdx.x;
  const EnvView v = env_view(d, b);
  const double a = v.rho / v.dt, mu = v.mu;
  extern __shared__ __align__(16) unsigned char setup_lds[];
  double* sGeo = reinterpret_cast<double*>(setup_lds);             // [5][NT]   (GEO)
  double* sGx = sGeo + (GEO ? 5 * (size_t)d.NT : 0);                // [N2]      (GEO)
  double* sSd = sGx + (GEO ? d.N2 : 0);                             // [NV]
  uint16_t* sCd = reinterpret_cast<uint16_t*>(sSd + d.NV);          // [6][NT]
  uint8_t* sFl = reinterpret_cast<uint8_t*>(sCd + 6 * (size_t)d.NT);  // [N2]
  uint8_t* sPf = sFl + d.N2;                                        // [NV]
  uint16_t* sG2p = reinterpret_cast<uint16_t*>(sPf + d.NV + ((d.N2 + d.NV) & 1));   // [N2 + 1]  (LS)
  uint16_t* sG2s = sG2p + d.N2 + 1;                                 // [6 NT]
  uint16_t* sG1p = sG2s + 6 * (size_t)d.NT;                         // [NV + 1]
  uint16_t* sG1s = sG1p + d.NV + 1;                                 // [3 NT]
  auto g2p = [&](int i) -> int { return LS ? (int)sG2p[i] : v.g2_ptr[i]; };
  auto g2s = [&](int i) -> int { return LS ? (int)sG2s[i] : v.g2_src[i]; };
  auto g1p = [&](int i) -> int { return LS ? (int)sG1p[i] : v.g1_ptr[i]; };
  auto g1s = [&](int i) -> int { return LS ? (int)sG1s[i] : v.g1_src[i]; };
  auto geo = [&](int e) -> Geo {
    if (!GEO) return load_geo(v, e);
    Geo g;
    g.j00 = sGeo[0 * v.NT + e];
    g.j01 = sGeo[1 * v.NT + e];
    g.j10 = sGeo[2 * v.NT + e];
    g.j11 = sGeo[3 * v.NT + e];
    g.det = sGeo[4 * v.NT + e];
    return g;
  };
  auto cdof = [&](int j, int e) -> int { return ST ? (int)sCd[j * v.NT + e] : v.cell_dofs[j * v.NT + e]; };
  auto uflag = [&](int i) -> bool { return ST ? sFl[i] != 0 : v.bcu_flag[i] != 0; };
  auto ugx = [&](int i) -> double { return GEO ? sGx[i] : v.bcu_gx[i]; };
  auto pflag = [&](int i) -> bool { return ST ? sPf[i] != 0 : v.bcp_flag[i] != 0; };
  auto sdk = [&](int i) -> double { return ST ? sSd[i] : v.sdiagK[i]; };
  if (ST) {
    for (int j = 0; j < 6; ++j)
      for (int e = tid; e < v.nt; e += SWG) sCd[j * v.NT + e] = (uint16_t)v.cell_dofs[j * v.NT + e];
    for (int i = tid; i < v.n2; i += SWG) {
      sFl[i] = v.bcu_flag[i];
      if (GEO) sGx[i] = v.bcu_gx[i];
    }
    for (int i = tid; i < v.nv; i += SWG) sPf[i] = v.bcp_flag[i];
    if (LS) {
      for (int i = tid; i <= v.n2; i += SWG) sG2p[i] = (uint16_t)v.g2_ptr[i];
      for (int i = tid; i < 6 * v.nt; i += SWG) sG2s[i] = (uint16_t)v.g2_src[i];
      for (int i = tid; i <= v.nv; i += SWG) sG1p[i] = (uint16_t)v.g1_ptr[i];
      for (int i = tid; i < 3 * v.nt; i += SWG) sG1s[i] = (uint16_t)v.g1_src[i];
    }
  }
  // reference-element tables in LDS: the row loops index them with the (lane-dependent) local row of a slot; from
  // constant memory that is one more dependent round trip per local column inside the conditional column loop
  __shared__ double sMhat[6][6];
  __shared__ double sGhat[2][2][6][6];
  for (int q = tid; q < 36; q += SWG) sMhat[q / 6][q % 6] = c_tab.Mhat[q / 6][q % 6];
  for (int q = tid; q < 144; q += SWG) sGhat[q / 72][(q / 36) % 2][(q / 6) % 6][q % 6] = c_tab.Ghat[q / 72][(q / 36) % 2][(q / 6) % 6][q % 6];
#ifdef MDQ_SETUP_TRACE
  long long tq_ = __builtin_amdgcn_s_memtime();
#endif
  for (int e = tid; e < v.nt; e += SWG) {
    double X[3][2];
    load_cell_coords(v, e, X);
    const double J00 = X[1][0] - X[0][0], J01 = X[2][0] - X[0][0];
    const double J10 = X[1][1] - X[0][1], J11 = X[2][1] - X[0][1];
    const double det = J00 * J11 - J01 * J10;
    const double q0 = J11 / det, q1 = -J01 / det, q2 = -J10 / det, q3 = J00 / det, q4 = fabs(det);
    v.geom[0 * v.NT + e] = q0;
    v.geom[1 * v.NT + e] = q1;
    v.geom[2 * v.NT + e] = q2;
    v.geom[3 * v.NT + e] = q3;
    v.geom[4 * v.NT + e] = q4;
    if (GEO) {
      sGeo[0 * v.NT + e] = q0;
      sGeo[1 * v.NT + e] = q1;
      sGeo[2 * v.NT + e] = q2;
      sGeo[3 * v.NT + e] = q3;
      sGeo[4 * v.NT + e] = q4;
    }
  }
  __syncthreads();
  ST_STAMP(0)
  if (v.nbo > 0) {
    const int nbe = v.bo_ptr[v.nbo];
    for (int t = tid; t < nbe; t += SWG) {
      const int slot = v.bo_src[t];
      const int e = slot / 36, ij = slot - e * 36, i = ij / 6, j = ij - i * 6;
      const Geo g = load_geo(v, e);
      double Bcd[2][2];
      outflow_entry(v, e, v.cell_outflow[e], i, j, g, Bcd);
      reinterpret_cast<double4*>(v.bo_val)[t] = make_double4(Bcd[0][0], Bcd[0][1], Bcd[1][0], Bcd[1][1]);
    }
  }
  ST_STAMP(1)
  // ---- P2 rows: raw diagonals (kept in idiag1 / sdiagM until the outflow rows have been corrected) and lifts
  for (int r = tid; r < v.n2; r += SWG) {
    double l1x = 0.0, l1y = 0.0, l3x = 0.0, dx = 0.0, dy = 0.0, dm = 0.0;
    // incident cells two at a time: the four dependent load levels of a cell (slot -> geometry / dofs -> Dirichlet
    // flags -> values) are paid once per pair; the second cell of an odd tail is the first one again, not added
    const int s0 = g2p(r), s1 = g2p(r + 1);
    for (int s = s0; s < s1; s += 2) {
      const bool two = s + 1 < s1;
      int ee[2], ii[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int slot = g2s((u == 1 && two) ? s + 1 : s);
        ee[u] = slot / 6;
        ii[u] = slot - ee[u] * 6;
      }
      Geo gg[2];
      int cj[2][6];
      bool fj[2][6];
      double gj[2][6];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        gg[u] = geo(ee[u]);
#pragma unroll
        for (int j = 0; j < 6; ++j) cj[u][j] = cdof(j, ee[u]);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 6; ++j) fj[u][j] = uflag(cj[u][j]);
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 6; ++j) gj[u][j] = ugx(cj[u][j]);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (u == 1 && !two) break;
        const Geo g = gg[u];
        const int i = ii[u];
        const double Ja[2][2] = {{g.j00, g.j01}, {g.j10, g.j11}};
        // The diagonal term with the tables indexed by the lane's own i: ONE block for the wave.  (As a column loop
        // unrolled over j with `if (j != i && !fc) continue` the wave ran all six blocks - its lanes sit at different i -
        // i.e. ~270 fp64 instructions per cell for one term per lane.)  The Dirichlet columns follow in ascending j as
        // before; only waves that hold cells at the boundary enter those blocks.
        {
          const double m = g.det * sMhat[i][i];
          const double g00 = sGhat[0][0][i][i], g01 = sGhat[0][1][i][i];
          const double g10 = sGhat[1][0][i][i], g11 = sGhat[1][1][i][i];
          const double kxx = g.det * (Ja[0][0] * (Ja[0][0] * g00 + Ja[1][0] * g01) + Ja[1][0] * (Ja[0][0] * g10 + Ja[1][0] * g11));
          const double kyy = g.det * (Ja[0][1] * (Ja[0][1] * g00 + Ja[1][1] * g01) + Ja[1][1] * (Ja[0][1] * g10 + Ja[1][1] * g11));
          const double L = kxx + kyy;
          dx += a * m + 0.5 * mu * (L + kxx);
          dy += a * m + 0.5 * mu * (L + kyy);
          dm += m;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          if (!fj[u][j]) continue;
          const double m = g.det * sMhat[i][j];
          const double g00 = sGhat[0][0][i][j], g01 = sGhat[0][1][i][j];
          const double g10 = sGhat[1][0][i][j], g11 = sGhat[1][1][i][j];
          const double kxx = g.det * (Ja[0][0] * (Ja[0][0] * g00 + Ja[1][0] * g01) + Ja[1][0] * (Ja[0][0] * g10 + Ja[1][0] * g11));
          const double kxy = g.det * (Ja[0][0] * (Ja[0][1] * g00 + Ja[1][1] * g01) + Ja[1][0] * (Ja[0][1] * g10 + Ja[1][1] * g11));
          const double kyy = g.det * (Ja[0][1] * (Ja[0][1] * g00 + Ja[1][1] * g01) + Ja[1][1] * (Ja[0][1] * g10 + Ja[1][1] * g11));
          const double L = kxx + kyy;
          const double bx = a * m + 0.5 * mu * (L + kxx), bz = 0.5 * mu * kxy;
          const double gx = gj[u][j];
          l1x += bx * gx;
          l1y += bz * gx;
          l3x += m * gx;
        }
      }
    }
    v.lift1[r] = make_double2(l1x, l1y);
    v.lift3[r] = make_double2(l3x, 0.0);
    v.idiag1[r] = make_double2(dx, dy);
    v.sdiagM[r] = dm;
  }
  __syncthreads();
  ST_STAMP(2)
  // outflow rows: - mu/2 B on the diagonal and in the lifts (one thread per row: no conflicts)
  for (int t = tid; t < v.nbo; t += SWG) {
    const int row = v.bo_rows[t];
    double2 dg = v.idiag1[row], l1 = v.lift1[row];
    for (int k = v.bo_ptr[t]; k < v.bo_ptr[t + 1]; ++k) {
      const double4 bv = reinterpret_cast<const double4*>(v.bo_val)[k];
      const int c = v.bo_col[k];
      if (c == row) {
        dg.x -= 0.5 * mu * bv.x;
        dg.y -= 0.5 * mu * bv.w;
      }
      if (uflag(c)) {
        const double gx = ugx(c);
        l1.x -= 0.5 * mu * bv.x * gx;
        l1.y -= 0.5 * mu * bv.z * gx;
      }
    }
    v.idiag1[row] = dg;
    v.lift1[row] = l1;
  }
  __syncthreads();
  for (int r = tid; r < v.n2; r += SWG) {
    const bool fr = uflag(r);
    const double2 dg = v.idiag1[r];
    v.idiag1[r] = fr ? make_double2(1.0, 1.0) : make_double2(1.0 / dg.x, 1.0 / dg.y);
    v.sdiagM[r] = fr ? 1.0 : sqrt(v.sdiagM[r]);
  }
  ST_STAMP(3)
  // ---- P1 Laplacian: entry (r, c) = sum over the cells of r that contain c of |T| grad(l_r).grad(l_c)
  auto k1_entry = [&](int r, int c) {
    double kk = 0.0;
    for (int s = g1p(r); s < g1p(r + 1); ++s) {
      const int slot = g1s(s);
      const int e = slot / 3, i = slot - e * 3;
      int j = -1;
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (cdof(q, e) == c) j = q;
      if (j < 0) continue;
      const Geo g = geo(e);
      const double dix = sel3(i, -g.j00 - g.j10, g.j00, g.j10), diy = sel3(i, -g.j01 - g.j11, g.j01, g.j11);
      const double djx = sel3(j, -g.j00 - g.j10, g.j00, g.j10), djy = sel3(j, -g.j01 - g.j11, g.j01, g.j11);
      kk += 0.5 * g.det * (dix * djx + diy * djy);
    }
    return kk;
  };
  for (int r = tid; r < v.nv; r += SWG) {
    const double sd = pflag(r) ? 1.0 : sqrt(k1_entry(r, r));
    v.sdiagK[r] = sd;
    if (ST) sSd[r] = sd;
  }
  __syncthreads();
  ST_STAMP(4)
  const int rows1 = ((v.nv + 63) >> 6) << 6;
  constexpr int KW = 16;   // widest row handled by the one-pass path (vertex degree + 1; wider rows: generic path)
  for (int r = tid; r < rows1; r += SWG) {
    const int off = v.sl1_off[r >> 6];
    const int width = (v.sl1_off[(r >> 6) + 1] - off) >> 6;
    if (width <= KW) {
      // ONE pass over the cells of the row: every cell adds its three entries (r, c_q) to the row's column list held in
      // registers (the generic path walks all cells of the row again for every entry: 7x the dependent loads; it
      // was 47 % of this kernel).  Same contributions in the same (cell) order per entry: same bits.
      int cols[KW];
      double vals[KW];
      int prev = -1;
#pragma unroll
      for (int j = 0; j < KW; ++j) {
        int c = -1;
        if (j < width && r < v.nv) {
          c = v.sl1_col[off + j * 64 + (r & 63)];
          if (c > prev) prev = c; else c = -1;   // (columns ascend; the padding repeats the row index)
        }
        cols[j] = c;
        vals[j] = 0.0;
      }
      if (r < v.nv) {
        if (pflag(r)) {
#pragma unroll
          for (int j = 0; j < KW; ++j) vals[j] = cols[j] == r ? 1.0 : 0.0;
        } else {
          for (int s_ = g1p(r); s_ < g1p(r + 1); ++s_) {
            const int slot = g1s(s_);
            const int e = slot / 3, i = slot - e * 3;
            const Geo g = geo(e);
            int cq[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) cq[q] = cdof(q, e);
            const double dix = sel3(i, -g.j00 - g.j10, g.j00, g.j10), diy = sel3(i, -g.j01 - g.j11, g.j01, g.j11);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              const double djx = sel3(q, -g.j00 - g.j10, g.j00, g.j10), djy = sel3(q, -g.j01 - g.j11, g.j01, g.j11);
              const double val = 0.5 * g.det * (dix * djx + diy * djy);
#pragma unroll
              for (int j = 0; j < KW; ++j) vals[j] += cols[j] == cq[q] ? val : 0.0;
            }
          }
          const double sr = sdk(r);
#pragma unroll
          for (int j = 0; j < KW; ++j) {
            if (cols[j] >= 0) {
              const int c = cols[j];
              vals[j] = pflag(c) ? (c == r ? 1.0 : 0.0) : vals[j] / (sr * sdk(c));
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < KW; ++j)
        if (j < width) v.K1s[off + j * 64 + (r & 63)] = cols[j] >= 0 ? vals[j] : 0.0;
      continue;
    }
    int prev = -1;
    for (int j = 0; j < width; ++j) {
      const int ps = off + j * 64 + (r & 63);
      double kk = 0.0;
      if (r < v.nv) {
        const int c = v.sl1_col[ps];
        if (c > prev) {  // real entry (columns ascend; the padding repeats the row index)
          prev = c;
          if (pflag(r) || pflag(c))
            kk = (c == r) ? 1.0 : 0.0;
          else
            kk = k1_entry(r, c) / (sdk(r) * sdk(c));
        }
      }
      v.K1s[ps] = kk;
    }
  }
  ST_STAMP(5)
}

}  // namespace mdq
