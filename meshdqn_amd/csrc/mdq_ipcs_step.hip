// IPCS, shared: the probes (forces), LdsPlan / lds_plan, the row groups and the phases of a time step, and what the entry
// unit shares with the team kernels (TEAM, team_cus).  Included by all four IPCS units, behind the pressure solvers.
namespace mdq {

// ================================================================== probes

// (drag, lift) of one field pair on the airfoil facets; result valid in every thread.
__device__ inline void forces(const EnvView& v, double mu, const double2* __restrict__ u,
                              const double* __restrict__ p, double* red, double& drag, double& lift) {
  double acc[2] = {0.0, 0.0};
  for (int f = threadIdx.x; f < v.naf; f += WG) {
    const int e = v.af_facets[2 * f], k = v.af_facets[2 * f + 1];
    const ElemIdx E = load_dofs(v, e);
    double X[3][2];
    load_cell_coords(v, e, X);
    // geometry straight from the coordinates: the probes then need no assembled operators
    // (Env2DAirfoil.calculate_reward samples them on every freshly coarsened mesh)
    Geo g;
    {
      const double J00 = X[1][0] - X[0][0], J01 = X[2][0] - X[0][0];
      const double J10 = X[1][1] - X[0][1], J11 = X[2][1] - X[0][1];
      const double det = J00 * J11 - J01 * J10;
      g.j00 = J11 / det;
      g.j01 = -J01 / det;
      g.j10 = -J10 / det;
      g.j11 = J00 / det;
      g.det = fabs(det);
    }
    const Facet F = facet_geometry(X, k);
    double2 ue[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) ue[i] = u[E.dof[i]];
    double pe[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pe[i] = p[E.dof[i]];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const double s = (q == 0 ? 0.5 - 0.28867513459481288225 : 0.5 + 0.28867513459481288225), w = 0.5 * F.len;
      const double xi = F.ra[0] + s * (F.rb[0] - F.ra[0]);
      const double eta = F.ra[1] + s * (F.rb[1] - F.ra[1]);
      double phi[6], dphi[6][2];
      p2_eval(xi, eta, phi, dphi);
      double uxx = 0, uxy = 0, uyx = 0, uyy = 0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double gx = g.j00 * dphi[j][0] + g.j10 * dphi[j][1];
        const double gy = g.j01 * dphi[j][0] + g.j11 * dphi[j][1];
        uxx += ue[j].x * gx;
        uxy += ue[j].x * gy;
        uyx += ue[j].y * gx;
        uyy += ue[j].y * gy;
      }
      const double pq = pe[0] * (1.0 - xi - eta) + pe[1] * xi + pe[2] * eta;
      const double sxx = 2.0 * mu * uxx - pq, sxy = mu * (uxy + uyx), syy = 2.0 * mu * uyy - pq;
      acc[0] += w * (sxx * F.nx + sxy * F.ny);
      acc[1] += w * (sxy * F.nx + syy * F.ny);
    }
  }
  block_sum<2>(acc, red);
  drag = acc[0];
  lift = acc[1];
}

// ================================================================== time stepping

#ifdef MDQ_PROFILE
#define MDQ_STAMP(k) { __syncthreads(); long long tn = __builtin_amdgcn_s_memtime(); prof[k] += tn - tprev; tprev = tn; }
#else
#define MDQ_STAMP(k)
#endif

// dynamic LDS: [red 64 doubles][union: velocity stage (MODE 1: p,r  double2[N2p] each;
//                                          evolve_mf_kernel: x stage double2[N2p] + element tile double2[6*WG])
//                                  | pressure: 4 vectors [NVp] + K1 in SELL form (values, columns, slice offsets)]
struct LdsPlan {
  int N2p, NVp;
  size_t vel1_bytes, vel2_bytes, vel3_bytes, prs_vec_bytes, prs_mat_bytes;
};
__host__ __device__ inline LdsPlan lds_plan(int N2, int NV, int NSE1) {
  LdsPlan P;
  P.N2p = (N2 + 1) & ~1;
  P.NVp = ((NV > 1024 ? NV : 1024) + 63) & ~63;  // (>= the 1024 threads of the direct pressure kernel)
  P.vel1_bytes = 2 * sizeof(double2) * (size_t)P.N2p;
  P.vel2_bytes = sizeof(double2) * ((size_t)P.N2p + 6 * MF_CH);  // stage + tile
  P.vel3_bytes = 3 * sizeof(double2) * (size_t)P.N2p;  // p, r, result vector
  P.prs_vec_bytes = 5 * sizeof(double) * (size_t)P.NVp;  // x, r, p, q + one scratch vector (direct solver)
  P.prs_mat_bytes = sizeof(double) * (size_t)(NSE1 > WG ? NSE1 : WG) + sizeof(int32_t) * ((size_t)NSE1 + (NSE1 & 1)) +
                    sizeof(int32_t) * (size_t)(((NV / 64 + 2) + 1) & ~1);
  return P;
}

// ------------------------------------------------------------------ the row phases of a time step
//
// Written once over a row group and an operator application (see "Krylov solvers"): evolve_kernel and the two team
// kernels call them.  What stays with each kernel: its row ranges and barriers (the group), who runs the pressure solve,
// where it keeps rho / dt, mu and the inflow factor, and - team kernels - the time-out handling.

// the last five tentative velocities (h1 = newest) and their count, in the environment's workspace slab
struct VelHist {
  double2 *h1, *h2, *h3, *h4, *h5;
  double* cnt;   // [0]: tentative velocities stored  ([1]: evolve_mf_kernel's corrections stored)
};
__device__ __forceinline__ VelHist vel_hist(const mdq_ipcs_desc& d, double* w) {
  VelHist H;
  H.h1 = reinterpret_cast<double2*>(w + work_hist_offset(d.NV, d.NT, d.NE));
  H.h2 = H.h1 + d.N2;
  H.h3 = H.h2 + d.N2;
  H.h4 = H.h3 + d.N2;
  H.h5 = H.h4 + d.N2;
  H.cnt = reinterpret_cast<double*>(H.h5 + d.N2);
  return H;
}

// initial guess of the velocity solve in row i: polynomial extrapolation in time of the previous tentative velocities
// h1 = u*_n .. h5 (the correction solve re-uses xs, so the history is kept separately; see at_velocity_kernel), `un` = u_n
// while there is no history
__device__ __forceinline__ double2 extrapolate_x0(int nhist, double2 un, const VelHist& H, int i) {
  double2 x0 = un;
  if (nhist >= 2) {
    const double2 us1 = H.h1[i], us2 = H.h2[i];
    x0 = make_double2(2.0 * us1.x - us2.x, 2.0 * us1.y - us2.y);
    if (nhist >= 3) {
      const double2 us3 = H.h3[i];
      x0 = make_double2(3.0 * (us1.x - us2.x) + us3.x, 3.0 * (us1.y - us2.y) + us3.y);
      if (nhist >= 4) {
        const double2 us4 = H.h4[i];
        x0 = make_double2(4.0 * (us1.x + us3.x) - 6.0 * us2.x - us4.x, 4.0 * (us1.y + us3.y) - 6.0 * us2.y - us4.y);
        if (nhist >= 5) {
          const double2 us5 = H.h5[i];
          x0 = make_double2(5.0 * (us1.x - us4.x) - 10.0 * (us2.x - us3.x) + us5.x,
                            5.0 * (us1.y - us4.y) - 10.0 * (us2.y - us3.y) + us5.y);
        }
      }
    }
  }
  return x0;
}
// shift the history of row i, newest first: h1 = u* of this step (xs)
__device__ __forceinline__ void history_shift(int nhist, const VelHist& H, const double2* xs, int i) {
  if (nhist >= 4) H.h5[i] = H.h4[i];
  if (nhist >= 3) H.h4[i] = H.h3[i];
  if (nhist >= 2) H.h3[i] = H.h2[i];
  if (nhist >= 1) H.h2[i] = H.h1[i];
  H.h1[i] = xs[i];
}

// row i of an element right-hand side: the sum of its slots of the element scratch, in list order
__device__ __forceinline__ double2 gather_slots2(const EnvView& v, const double2* escr2, int i) {
  double2 f = make_double2(0.0, 0.0);
  for (int s = v.g2_ptr[i]; s < v.g2_ptr[i + 1]; ++s) {
    const double2 c = escr2[v.g2_src[s]];
    f.x += c.x;
    f.y += c.y;
  }
  return f;
}

// Step 1 behind the element loop: right-hand side rows b = D^-1 (f - ai lift1) (Dirichlet rows: ai g), initial guess x0 in
// c.x, initial residual r0 = b - (D^-1 A) x0 in c.r / c.rh, p = v = 0; acc = { |b|^2, |r0|^2 } on exit.
// TILE: the operator is the full element operator (no lifting vector: x0 carries the Dirichlet values), so the residual
// is seeded with D^-1 f and zeros on constrained rows; |b|^2 is the assembled modes' either way.
template <bool TILE, class RG, class Op>
__device__ __forceinline__ void velocity_rhs(const RG& rg, const Op& apply, const EnvView& v, const VelCtx& c, double ai,
                                             const double2* escr2, int nhist, const VelHist& H, double* red, double (&acc)[2]) {
  rg.rows(v.n2, [&](int i) {
    const double2 f = gather_slots2(v, escr2, i);
    const double2 l = scaled2(ai, v.lift1[i]), id = v.idiag1[i];
    const bool fl = v.bcu_flag[i] != 0;
    const double2 g = make_double2(ai * v.bcu_gx[i], 0.0);
    const double2 bi = fl ? g : make_double2((f.x - l.x) * id.x, (f.y - l.y) * id.y);
    double2 x0 = extrapolate_x0(nhist, v.u_n[i], H, i);
    if (fl) x0 = g;   // Dirichlet values hold
    c.x[i] = x0;
    if (TILE)
      c.r[i] = fl ? make_double2(0.0, 0.0) : make_double2(f.x * id.x, f.y * id.y);
    else
      c.r[i] = bi;
    acc[0] += bi.x * bi.x + bi.y * bi.y;
  });
  rg.sync();
  apply(c.x, [&](int row, double y0, double y1) {
    const double2 bi = c.r[row];
    const double2 r0 = make_double2(bi.x - y0, bi.y - y1);
    c.r[row] = r0;
    c.rh[row] = r0;
    c.p[row] = make_double2(0.0, 0.0);
    c.vv[row] = make_double2(0.0, 0.0);
    acc[1] += r0.x * r0.x + r0.y * r0.y;
  });
  rg.sum(acc, red);
}

// the pressure vectors and the K1 stage of the kernels' LDS union (see LdsPlan)
struct PrsLds {
  double *x, *r, *p, *q, *lK;   // lK [NSE1] (K1_LDS; the direct solver's scratch vector otherwise)
  int32_t *lci, *lso;           // [NSE1], [NV/64+2]
};
__device__ __forceinline__ PrsLds prs_lds(double* U, const LdsPlan& P, const mdq_ipcs_desc& d) {
  PrsLds L;
  L.x = U;
  L.r = L.x + P.NVp;
  L.p = L.r + P.NVp;
  L.q = L.p + P.NVp;
  L.lK = L.q + P.NVp;
  L.lci = reinterpret_cast<int32_t*>(L.lK + d.NSE1);
  L.lso = L.lci + d.NSE1 + (d.NSE1 & 1);
  return L;
}

// what pressure_krylov_lds takes behind its vectors: each kernel's own (scratch room, tables, the on-chip solver's union)
struct KrylovLds {
  size_t scratch_bytes;
  double* extra;
  size_t extra_bytes;
  double* U;
  size_t U_bytes;
  int NVp;
};

// Step 2 behind the element loop, by ONE workgroup: K1 into LDS (K1_LDS), right-hand side rows and the scaled start vector,
// the direct solve where this environment has factors (DIRECT) or the Krylov solve (its iterations are returned),
// pnew = S^-1 x.  `stamp`: the profile build's phase stamps 3 / 4.  (`red` is a plain argument, not a member of a struct:
// the out-of-line pressure solvers are compiled knowing that it is the start of the LDS only while every caller hands the
// constant down through arguments.)
template <bool K1_LDS, bool DIRECT, class Stamp>
__device__ __forceinline__ int pressure_solve(const EnvView& v, const mdq_ipcs_desc& d, int b, const double* escr1, const PrsLds& L,
                                              double* pnew, const KrylovLds& ka, double* red, const Stamp& stamp) {
  const int tid = threadIdx.x, nv = v.nv;
  const int nsl1 = (nv + 63) >> 6;
  const int32_t* so1 = K1_LDS ? L.lso : v.sl1_off;
  const int32_t* ci1 = K1_LDS ? L.lci : v.sl1_col;
  const double* K1 = K1_LDS ? L.lK : v.K1s;
  int it = 0;
  if (K1_LDS && !d.pd_enabled) {
    const int ne1 = v.sl1_off[nsl1];
    for (int k = tid; k < ne1; k += WG) {
      L.lK[k] = v.K1s[k];
      L.lci[k] = v.sl1_col[k];
    }
    for (int k = tid; k <= nsl1; k += WG) L.lso[k] = v.sl1_off[k];
  }
  for (int i = tid; i < nv; i += WG) {
    double bsum = 0.0;
    for (int s = v.g1_ptr[i]; s < v.g1_ptr[i + 1]; ++s) bsum += escr1[v.g1_src[s]];
    const double sd = v.sdiagK[i];
    L.r[i] = v.bcp_flag[i] ? 0.0 : bsum / sd;
    L.x[i] = v.p_n[i] * sd;
  }
  stamp(3);
  if (DIRECT && d.pd_enabled && d.pd_hdr[4 * (int64_t)b + 2] > 0) {   // (nparts = 0: no factors for this environment -> Krylov)
    const PdView pd = pd_view(d, b);
    pressure_direct(pd, nv, L.r, L.x, L.p, L.q, L.lK);
  } else {
    it = pressure_krylov_lds(d, K1_LDS, nv, so1, ci1, K1, v.coords, L.x, L.r, L.p, L.q, ka.scratch_bytes, ka.extra, ka.extra_bytes, red,
                             ka.U, ka.U_bytes, ka.NVp);
  }
  stamp(4);
  for (int i = tid; i < nv; i += WG) pnew[i] = L.x[i] / v.sdiagK[i];
  return it;
}

// Step 3 behind the element loop: right-hand side rows b = S^-1 (f - ai lift3) (Dirichlet rows: ai g), the scaled unknown
// S x0 in c.x, r0 = b - (S^-1 M S^-1)(S x0) in c.r, p0 = r0; am = { |b|^2, |r0|^2 } on exit.  TILE: as in velocity_rhs, and
// the operator gathers S^-1 (.) from the stage c.gp: x0 for the residual, then S^-1 p0 for the solver (staged behind the
// reduction's barrier: every gather of x0 is complete).
template <bool TILE, class RG, class Op>
__device__ __forceinline__ void correction_rhs(const RG& rg, const Op& apply, const EnvView& v, const MassCtx& c, double ai,
                                               const double2* escr2, double* red, double (&am)[2]) {
  rg.rows(v.n2, [&](int i) {
    const double2 f = gather_slots2(v, escr2, i);
    const double2 l = scaled2(ai, v.lift3[i]);
    const double sd = v.sdiagM[i];
    const bool fl = v.bcu_flag[i] != 0;
    const double2 g = make_double2(ai * v.bcu_gx[i], 0.0);
    const double2 bi = fl ? g : make_double2((f.x - l.x) / sd, (f.y - l.y) / sd);
    double2 x0 = c.x[i];
    if (fl) x0 = g;   // (not `fl ? g : c.x[i]`: a choice between two objects keeps g in scratch memory)
    c.x[i] = make_double2(x0.x * sd, x0.y * sd);  // scaled unknown S x
    if (TILE) {
      c.gp[i] = x0;  // S^-1 (S x0)
      c.r[i] = fl ? make_double2(0.0, 0.0) : make_double2(f.x / sd, f.y / sd);
    } else {
      c.r[i] = bi;
    }
    am[0] += bi.x * bi.x + bi.y * bi.y;
  });
  rg.sync();
  apply(TILE ? c.gp : c.x, [&](int row, double y0, double y1) {
    const double2 bi = c.r[row];
    const double2 r0 = make_double2(bi.x - y0, bi.y - y1);
    c.r[row] = r0;
    c.p[row] = r0;
    am[1] += r0.x * r0.x + r0.y * r0.y;
  });
  rg.sum(am, red);
  if (TILE) {
    rg.rows(v.n2, [&](int i) {
      const double is = 1.0 / v.sdiagM[i];
      const double2 p0 = c.p[i];
      c.gp[i] = make_double2(p0.x * is, p0.y * is);
    });
    rg.sync();
  }
}

// u_n = S^-1 (S x) on the group's rows
template <class RG>
__device__ __forceinline__ void update_velocity(const RG& rg, const EnvView& v, const double2* xs) {
  rg.rows(v.n2, [&](int i) {
    const double sd = v.sdiagM[i];
    const double2 x = xs[i];
    v.u_n[i] = make_double2(x.x / sd, x.y / sd);
  });
}

// workgroups per environment of the team modes 4 / 7 (mdq_ipcs_team.hip; the entry unit's automatic mode choice reads it)
constexpr int TEAM = 2;

// CUs the team modes may count on when they are chosen AUTOMATICALLY: every workgroup of a team must be resident at the same
// time (the barrier spins), so the launch stream has to own that many CUs - the CUs of the stream's mask when it carries one
// (hipExtStreamCreateWithCUMask: meshdqn_amd/streams.py, MDQ_CU_PARTITION), and none at all when the process has been told
// that it shares the GPU with other processes (MDQ_SHARE_GPU: several ranks on one device).  An explicit mode 4 / 7 is the
// caller's decision; a time-out is reported either way (team_failed).
static int team_cus(hipStream_t st) {
  static const int ncu = [] {
    int dev_ = 0, n_ = 0;
    if (hipGetDevice(&dev_) != hipSuccess || hipDeviceGetAttribute(&n_, hipDeviceAttributeMultiprocessorCount, dev_) != hipSuccess)
      return 0;
    return n_;
  }();
  if (std::getenv("MDQ_SHARE_GPU") != nullptr) return 0;
  uint32_t mask[16] = {0};
  if (hipExtStreamGetCUMask(st, 16, mask) != hipSuccess) {
    (void)hipGetLastError();
    return ncu;
  }
  int n = 0;
  for (int i = 0; i < 16; ++i) n += __builtin_popcount(mask[i]);
  return n > 0 && n < ncu ? n : ncu;
}

}  // namespace mdq
