// IPCS: the matrix-free mode 2 with the Krylov vectors in registers - opaque_lane, MDQ_FOR_ROWS, evolve_mf_kernel (three
// launches per step) and launch_evolve_mf.  Included by mdq_tu_ipcs_mf.hip only, behind the phases of a time step.
namespace mdq {

// ================================================================== matrix-free kernel, Krylov vectors in registers
//
// MODE 2 proper: every thread keeps its own rows (tid + k*WG, k < MF_ROWS) of ALL Krylov vectors
// in registers for the whole solve; per operator application only the gather copy of the input
// vector goes through LDS (stage) and the element results through the LDS tile.  Global memory is
// touched only for the element metadata (dofs, tile maps, geometry) and once per time step for
// the state vectors.

// a lane index the compiler cannot see through: the per-row addresses (7 rows x 6 slab vectors x 64 bits) are then
// computed where they are used - hoisted out of the Krylov loop they were what the register allocator spilled
__device__ __forceinline__ int opaque_lane(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

#define MDQ_FOR_ROWS(k, row)                       \
  _Pragma("unroll") for (int k = 0; k < MF_ROWS; ++k) \
    if (const int row = threadIdx.x + k * WG; row < n2)

// Round 5: ONE STEP = THREE LAUNCHES (PHASE 1 tentative velocity, 2 pressure, 3 correction + probes), like mode 3.  The
// persistent kernel of rounds 1-4 (all steps in one launch, r / p / v / t of the BiCGStab solve and x / r / p / q of the mass CG
// in registers across the element phases) sat at 256 VGPRs + 836-932 B per lane of scratch: every operator application
// spilled and re-read ~200 dwords per lane, 428 KB per workgroup, around a phase that needs ~100 registers of its own.  Now
// every phase has its own register allocation, and across an operator application only what the application cannot get
// elsewhere stays in registers: the residual r (+ the fp32 row scaling).  The search direction p is in LDS anyway while it is
// applied (the gather copy `stage`: the owner reads its rows back from there) and, like v = A p and the iterate x, has a
// row-owner-only copy in the environment's workspace slab (coalesced 16-byte accesses that stay in L2): 4 vector passes of
// 53 KB per iteration instead of the scratch traffic.  Same operations on the same values in the same order as before
// (x += alpha p and x += omega s are the two fma's the old single expression contracted to): bitwise reproducible, and the
// element results still meet in the LDS tile in ascending triangle order.
template <bool K1_LDS, int PHASE>
__global__ __launch_bounds__(WG) void evolve_mf_kernel(mdq_ipcs_desc d, int nsteps, int step, double* drag, double* lift,
                                                        int32_t* iters, const double* inflow_scale) {
  extern __shared__ __align__(16) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const EnvView v = env_view(d, b);
  const double ai = inflow_factor(inflow_scale, b, nsteps, step);
  const int n2 = v.n2, nv = v.nv;
  const LdsPlan P = lds_plan(d.N2, d.NV, d.NSE1);

  double* red = smem;  // 64 doubles
  double* U = smem + 64;

  double* w = v.work;
  double* escr1 = w;
  double2* xs = reinterpret_cast<double2*>(w + 12 * (int64_t)d.NT);  // u* (the iterate of the velocity solve)
  double2* rhg = xs + d.N2;                                            // shadow residual; phase 3: predicted correction, then x
  double* pnew = reinterpret_cast<double*>(xs + 6 * (int64_t)d.N2);
  // initial guesses extrapolated in time: the last five tentative velocities (same slots and counter as evolve_kernel:
  // h1 = newest) and a ring of the last three velocity corrections u_{n+1} - u*.  Every row is read and written by its
  // owner only.
  const VelHist H = vel_hist(d, w);
  double* hcnt = H.cnt;   // [0]: tentative velocities stored, [1]: corrections stored
  double2* c1 = xs + 2 * (int64_t)d.N2;                  // newest correction
  double2* c2 = c1 + d.N2;
  double2* c3 = c2 + d.N2;
  double2* pg = c3 + d.N2;                                                              // search direction (own rows)
  double2* vg = reinterpret_cast<double2*>(w + work_ytmp_offset(d.NV, d.NT, d.NE));     // v = D^-1 A p (own rows)

  if constexpr (PHASE == 1) {
    // ================= step 1: tentative velocity
    const double a = v.rho / v.dt, mu = v.mu;
    double2* stage = reinterpret_cast<double2*>(U);  // gather copy of the operator input
    double2* tile = stage + P.N2p;                    // element results of one chunk
    double2* rg = reinterpret_cast<double2*>(w);     // (the element scratch of phase 2, idle here: room for the row scaling)
    TileMeta tm;
    tile_prefetch(v, tm, 0);
    int it_u = 0;
    double2 r[MF_ROWS];
    const int nhist = (int)hcnt[0];
    // Jacobi row scaling of the velocity system with the Dirichlet flag folded in (0 = constrained row), rounded to fp32
    // as in rounds 1-4 (any positive row scaling is a valid left preconditioner and the solution of D^-1 A x = D^-1 b does
    // not depend on it; the same values keep the trajectories of the committed fixtures) - now an own-row vector in the
    // slab like p and v: as a register array it was what the compiler spilled (36 dwords, re-read in every row loop)
    double2* idgg = rg;
#pragma unroll 1
    for (int row = tid; row < n2; row += WG) {
      double2 s_ = make_double2(0.0, 0.0);
      if (!v.bcu_flag[row]) {
        const double2 t_ = v.idiag1[row];
        s_ = make_double2((double)(float)t_.x, (double)(float)t_.y);
      }
      idgg[row] = s_;
    }
    // initial guess: u_n, or the polynomial extrapolation in time of the stored tentative velocities (evolve_kernel's
    // formulas); it satisfies the Dirichlet values
#pragma unroll 1
    for (int row = tid; row < n2; row += WG) {
      double2 x0 = extrapolate_x0(nhist, v.u_n[row], H, row);
      if (v.bcu_flag[row] != 0) x0 = make_double2(ai * v.bcu_gx[row], 0.0);
      xs[row] = x0;
      stage[row] = x0;
    }
    double acc[2] = {0.0, 0.0};
    {
      double2 y[MF_ROWS];
      {
        // f = rhs(F1) (volume + outflow facet term), element vectors through the tile
        const double2* un = v.u_n;
        const double* pn = v.p_n;
        tile_accumulate(
            v, tile, tm,
            [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
              double2 ue[6];
#pragma unroll
              for (int i = 0; i < 6; ++i) ue[i] = un[E.dof[i]];
              double pe[3];
#pragma unroll
              for (int i = 0; i < 3; ++i) pe[i] = pn[E.dof[i]];
              elem_rhs1_vol(g, a, mu, v.rho, ue, pe, ye);
              if (ko >= 0) {
                double X[3][2];
                load_cell_coords(v, e, X);
                elem_outflow_add(g, X, ko, 0.5 * mu, ue, ye);
              }
            },
            y);
      }
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        if (row < n2) {
          const bool fl = v.bcu_flag[row] != 0;
          const double2 g = make_double2(ai * v.bcu_gx[row], 0.0);
          // |D^-1 b|^2 with b = f - lift (free) / g (constrained): same norm as the assembled path
          const double2 l = scaled2(ai, v.lift1[row]);
          const double2 sc = idgg[row];
          const double2 bi = fl ? g : make_double2((y[k].x - l.x) * sc.x, (y[k].y - l.y) * sc.y);
          acc[0] += bi.x * bi.x + bi.y * bi.y;
        }
      }
      // (the tile_accumulate above ended with a barrier: the staged x0 of every row is visible)
      double2 ax[MF_ROWS];
      tile_accumulate(
          v, tile, tm,
          [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
            double2 xe[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) xe[i] = stage[E.dof[i]];
            velocity_op(v, a, mu, e, ko, g, xe, ye);
          },
          ax);
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        // r0 = D^-1 (f - A_full x0) on free rows, 0 on constrained rows (the scaling is 0 there)
        r[k] = make_double2(0.0, 0.0);
        if (row < n2) {
          const double2 sc = idgg[row];
          r[k] = make_double2((y[k].x - ax[k].x) * sc.x, (y[k].y - ax[k].y) * sc.y);
          rhg[row] = r[k];
          pg[row] = make_double2(0.0, 0.0);
          vg[row] = make_double2(0.0, 0.0);
        }
        acc[1] += r[k].x * r[k].x + r[k].y * r[k].y;
      }
    }
    block_sum<2>(acc, red);
    {
      const double bb = acc[0], tol2 = d.rtol * d.rtol * bb;
      double rr = acc[1];
      if (rr > tol2 && bb != 0.0) {
        double rho = rr, rho_old = 1.0, alpha = 1.0, omega = 1.0;
        int it = 0;
        while (it < d.maxit_u) {
          ++it;
          const double beta = (rho / rho_old) * (alpha / omega);
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const int row = opaque_lane(tid) + k * WG;
            if (row < n2) {
              const double2 po = pg[row], vo = vg[row];
              const double2 pk = make_double2(r[k].x + beta * (po.x - omega * vo.x), r[k].y + beta * (po.y - omega * vo.y));
              pg[row] = pk;
              stage[row] = pk;
            }
          }
          __syncthreads();
          double a1[1] = {0.0};
          double2 vv[MF_ROWS];                   // (live until s = r - alpha v below; its slab copy is for the next p update)
          {
            tile_accumulate(
                v, tile, tm,
                [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
                  double2 xe[6];
#pragma unroll
                  for (int i = 0; i < 6; ++i) xe[i] = stage[E.dof[i]];
                  velocity_op(v, a, mu, e, ko, g, xe, ye);
                },
                vv);
#pragma unroll
            for (int k = 0; k < MF_ROWS; ++k) {
              const int row = opaque_lane(tid) + k * WG;
              if (row < n2) {
                const double2 h = rhg[row], sc = idgg[row];
                vv[k] = make_double2(vv[k].x * sc.x, vv[k].y * sc.y);
                a1[0] += h.x * vv[k].x + h.y * vv[k].y;
                vg[row] = vv[k];
              }
            }
          }
          block_sum<1>(a1, red);
          if (a1[0] == 0.0) break;
          alpha = rho / a1[0];
          double a2[1] = {0.0};
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const int row = opaque_lane(tid) + k * WG;
            if (row < n2) {
              const double2 vo = vv[k], pk = stage[row], xo = xs[row];    // (own rows)
              r[k] = make_double2(r[k].x - alpha * vo.x, r[k].y - alpha * vo.y);  // s
              xs[row] = make_double2(xo.x + alpha * pk.x, xo.y + alpha * pk.y);
              stage[row] = r[k];
            }
            else
              r[k] = make_double2(0.0, 0.0);
            a2[0] += r[k].x * r[k].x + r[k].y * r[k].y;
          }
          block_sum<1>(a2, red);  // its barriers publish the staged s
          if (!(a2[0] > tol2)) break;            // (x = x + alpha p is already in place)
          double a3[2] = {0.0, 0.0};
          double2 t[MF_ROWS];
          tile_accumulate(
              v, tile, tm,
              [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
                double2 xe[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) xe[i] = stage[E.dof[i]];
                velocity_op(v, a, mu, e, ko, g, xe, ye);
              },
              t);
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const int row = opaque_lane(tid) + k * WG;
            const double2 sc = row < n2 ? idgg[row] : make_double2(0.0, 0.0);
            t[k] = make_double2(t[k].x * sc.x, t[k].y * sc.y);
            a3[0] += t[k].x * r[k].x + t[k].y * r[k].y;
            a3[1] += t[k].x * t[k].x + t[k].y * t[k].y;
          }
          block_sum<2>(a3, red);
          if (a3[1] == 0.0) break;
          omega = a3[0] / a3[1];
          double a4[2] = {0.0, 0.0};
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const int row = opaque_lane(tid) + k * WG;
            if (row < n2) {
              const double2 xo = xs[row], h = rhg[row];
              xs[row] = make_double2(xo.x + omega * r[k].x, xo.y + omega * r[k].y);
              r[k] = make_double2(r[k].x - omega * t[k].x, r[k].y - omega * t[k].y);
              a4[0] += r[k].x * r[k].x + r[k].y * r[k].y;
              a4[1] += h.x * r[k].x + h.y * r[k].y;
            }
          }
          block_sum<2>(a4, red);
          rr = a4[0];
          if (!(rr > tol2)) break;
          rho_old = rho;
          rho = a4[1];
          if (rho == 0.0 || omega == 0.0) break;
        }
        it_u += it;
      }
    }
#pragma unroll 1
    for (int row = tid; row < n2; row += WG) history_shift(nhist, H, xs, row);   // (own rows)
    if (tid == 0) hcnt[0] = (double)(nhist < 5 ? nhist + 1 : 5);
    if (tid == 0 && iters) iters[3 * b + 0] += it_u;
  } else if constexpr (PHASE == 2) {
    // ================= step 2: pressure (assembled K1 in SELL form, LDS resident)
    double* px = U;
    double* pr = px + P.NVp;
    double* pp = pr + P.NVp;
    double* pq = pp + P.NVp;
    double* lK = pq + P.NVp;
    int32_t* lci = reinterpret_cast<int32_t*>(lK + d.NSE1);
    int32_t* lso = lci + d.NSE1 + (d.NSE1 & 1);
    const int nsl1 = (nv + 63) >> 6;
    const int32_t* so1 = K1_LDS ? lso : v.sl1_off;
    const int32_t* ci1 = K1_LDS ? lci : v.sl1_col;
    const double* K1 = K1_LDS ? lK : v.K1s;
    int it_p = 0;
    if (K1_LDS && !d.pd_enabled) {
      const int ne1 = v.sl1_off[nsl1];
      for (int kk = tid; kk < ne1; kk += WG) {
        lK[kk] = v.K1s[kk];
        lci[kk] = v.sl1_col[kk];
      }
      for (int kk = tid; kk <= nsl1; kk += WG) lso[kk] = v.sl1_off[kk];
    }
    rhs2_elements(v, d, xs, v.p_n, escr1);
    __syncthreads();
    for (int i = tid; i < nv; i += WG) {
      double bsum = 0.0;
      for (int s = v.g1_ptr[i]; s < v.g1_ptr[i + 1]; ++s) bsum += escr1[v.g1_src[s]];
      const double sd = v.sdiagK[i];
      pr[i] = v.bcp_flag[i] ? 0.0 : bsum / sd;
      px[i] = v.p_n[i] * sd;
    }
    if (d.pd_enabled && d.pd_hdr[4 * (int64_t)b + 2] > 0) {   // (nparts = 0: no factors for this environment -> Krylov)
      const PdView pd = pd_view(d, b);
      pressure_direct(pd, nv, pr, px, pp, pq, lK);
    } else {
      it_p += cg_pressure(nv, so1, ci1, K1, d.rtol, d.maxit_p, px, pr, pp, pq, red);
    }
    for (int i = tid; i < nv; i += WG) pnew[i] = px[i] / v.sdiagK[i];
    if (tid == 0 && iters) iters[3 * b + 1] += it_p;
  } else {
    // ================= step 3: velocity correction (mass solve, both components)
    double2* stage = reinterpret_cast<double2*>(U);
    double2* tile = stage + P.N2p;
    double2* xg = rhg;              // the scaled unknown S x of the mass CG (own rows), once the predicted correction is consumed
    TileMeta tm;
    tile_prefetch(v, tm, 0);
    int it_m = 0;
    const int ncorr = (int)hcnt[1];
    double am[2] = {0.0, 0.0};
    double2 r[MF_ROWS], p[MF_ROWS];
    // symmetric Jacobi scaling S^-1 of the mass system, 0 on constrained rows
    double ism[MF_ROWS];
    {
      double2 y[MF_ROWS];
      {
        const double* pold = v.p_n;
        tile_accumulate(
            v, tile, tm,
            [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
              double2 ue[6];
#pragma unroll
              for (int i = 0; i < 6; ++i) ue[i] = xs[E.dof[i]];
              double dp[3];
#pragma unroll
              for (int i = 0; i < 3; ++i) dp[i] = pnew[E.dof[i]] - pold[E.dof[i]];
              elem_rhs3(g, v.dt, ue, dp, ye);
            },
            y);
      }
      double2 x[MF_ROWS];
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        // u* (own rows) + the correction extrapolated from the ring (0 on constrained rows: the corrections vanish there)
        x[k] = make_double2(0.0, 0.0);
        ism[k] = 0.0;
        if (row < n2) {
          double2 dp_ = make_double2(0.0, 0.0);
          if (ncorr >= 1) {
            const double2 d1 = c1[row];
            dp_ = d1;
            if (ncorr >= 2) {
              const double2 d2 = c2[row];
              dp_ = make_double2(2.0 * d1.x - d2.x, 2.0 * d1.y - d2.y);
              if (ncorr >= 3) {
                const double2 d3 = c3[row];
                dp_ = make_double2(3.0 * (d1.x - d2.x) + d3.x, 3.0 * (d1.y - d2.y) + d3.y);
              }
            }
          }
          const double2 us = xs[row];
          x[k] = make_double2(us.x + dp_.x, us.y + dp_.y);
          // x satisfies the Dirichlet values: scaled unknown S x, stage S^-1 (S x0) = x0
          const bool fl = v.bcu_flag[row] != 0;
          if (!fl) ism[k] = 1.0 / v.sdiagM[row];
          stage[row] = x[k];
          const double2 l = scaled2(ai, v.lift3[row]);
          const double2 bi = fl ? x[k] : make_double2((y[k].x - l.x) * ism[k], (y[k].y - l.y) * ism[k]);
          am[0] += bi.x * bi.x + bi.y * bi.y;
        }
      }
      __syncthreads();
      double2 ax[MF_ROWS];
      tile_accumulate(
          v, tile, tm,
          [&](int, const Geo& g, const ElemIdx& E, int, double2(&ye)[6]) {
            double2 xe[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) xe[i] = stage[E.dof[i]];
            elem_mass(g, xe, ye);
          },
          ax);
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        r[k] = make_double2((y[k].x - ax[k].x) * ism[k], (y[k].y - ax[k].y) * ism[k]);  // 0 on constrained rows
        p[k] = r[k];
        am[1] += r[k].x * r[k].x + r[k].y * r[k].y;
        // scaled unknown: S x (S = 1/ism on free rows; constrained rows keep x = g with S = 1)
        if (ism[k] != 0.0) x[k] = make_double2(x[k].x / ism[k], x[k].y / ism[k]);
        if (row < n2) xg[row] = x[k];
      }
    }
    block_sum<2>(am, red);
    {
      const double bb = am[0], tol2 = d.rtol * d.rtol * bb;
      double rr = am[1];
      if (rr > tol2 && bb != 0.0) {
        int it = 0;
        while (it < d.maxit_m) {
          ++it;
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const int row = tid + k * WG;
            if (row < n2) stage[row] = make_double2(p[k].x * ism[k], p[k].y * ism[k]);
          }
          __syncthreads();
          double2 q[MF_ROWS];
          tile_accumulate(
              v, tile, tm,
              [&](int, const Geo& g, const ElemIdx& E, int, double2(&ye)[6]) {
                double2 xe[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) xe[i] = stage[E.dof[i]];
                elem_mass(g, xe, ye);
              },
              q);
          double a1[1] = {0.0};
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            q[k] = make_double2(q[k].x * ism[k], q[k].y * ism[k]);
            a1[0] += p[k].x * q[k].x + p[k].y * q[k].y;
          }
          block_sum<1>(a1, red);
          if (!(a1[0] > 0.0)) break;
          const double alpha = rr / a1[0];
          double a2[1] = {0.0};
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const int row = tid + k * WG;
            if (row < n2) {
              const double2 xo = xg[row];
              xg[row] = make_double2(xo.x + alpha * p[k].x, xo.y + alpha * p[k].y);
            }
            r[k] = make_double2(r[k].x - alpha * q[k].x, r[k].y - alpha * q[k].y);
            a2[0] += r[k].x * r[k].x + r[k].y * r[k].y;
          }
          block_sum<1>(a2, red);
          const double rr_new = a2[0];
          if (!(rr_new > tol2)) break;
          const double beta = rr_new / rr;
          rr = rr_new;
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k)
            p[k] = make_double2(r[k].x + beta * p[k].x, r[k].y + beta * p[k].y);
        }
        it_m += it;
      }
    }

    // ================= update state + probes
#pragma unroll
    for (int k = 0; k < MF_ROWS; ++k) {
      const int row = tid + k * WG;
      if (row < n2) {
        const double2 xk = xg[row], us = xs[row];
        const double2 un = (ism[k] != 0.0) ? make_double2(xk.x * ism[k], xk.y * ism[k]) : xk;
        v.u_n[row] = un;
        // ring of corrections, newest first (own rows)
        if (ncorr >= 2) c3[row] = c2[row];
        if (ncorr >= 1) c2[row] = c1[row];
        c1[row] = make_double2(un.x - us.x, un.y - us.y);
      }
    }
    if (tid == 0) hcnt[1] = (double)(ncorr < 3 ? ncorr + 1 : 3);
    for (int i = tid; i < nv; i += WG) v.p_n[i] = pnew[i];
    __syncthreads();
    double dr, li;
    forces(v, v.mu, v.u_n, v.p_n, red, dr, li);
    if (tid == 0) {
      drag[(int64_t)b * nsteps + step] = dr;
      lift[(int64_t)b * nsteps + step] = li;
    }
    if (tid == 0 && iters) iters[3 * b + 2] += it_m;
  }
}

// the inflow profile of step `step` (mdq_ipcs_evolve_profile) in front of that step's kernels: defined in part 0, which
// owns inflow_lift_kernel; called from the per-step launch loops of modes 2 and 3
hipError_t launch_inflow_lift(const mdq_ipcs_desc* d, const mdq_inflow_profile* prof, int nsteps, int step, hipStream_t st);

template <bool K1_LDS>
static hipError_t launch_evolve_mf(const mdq_ipcs_desc* d, size_t lds, int nsteps, double* drag, double* lift,
                                   int32_t* iters, const double* inflow_scale, const mdq_inflow_profile* prof,
                                   hipStream_t stream) {
  static const hipError_t attr = [] {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&evolve_mf_kernel<K1_LDS, 1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&evolve_mf_kernel<K1_LDS, 2>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&evolve_mf_kernel<K1_LDS, 3>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return e;
  }();
  if (attr != hipSuccess) return attr;
  const LdsPlan P = lds_plan(d->N2, d->NV, d->NSE1);
  const size_t red_bytes = 64 * sizeof(double);
  const size_t lds_v = red_bytes + P.vel2_bytes;
  const size_t lds_p = red_bytes + P.prs_vec_bytes + (K1_LDS ? P.prs_mat_bytes : 0);
  (void)lds;
  for (int step = 0; step < nsteps; ++step) {
    if (prof)
      if (hipError_t e = launch_inflow_lift(d, prof, nsteps, step, stream); e != hipSuccess) return e;
    hipLaunchKernelGGL((evolve_mf_kernel<K1_LDS, 1>), dim3(d->B), dim3(WG), lds_v, stream, *d, nsteps, step, drag, lift, iters, inflow_scale);
    hipLaunchKernelGGL((evolve_mf_kernel<K1_LDS, 2>), dim3(d->B), dim3(WG), lds_p, stream, *d, nsteps, step, drag, lift, iters, inflow_scale);
    hipLaunchKernelGGL((evolve_mf_kernel<K1_LDS, 3>), dim3(d->B), dim3(WG), lds_v, stream, *d, nsteps, step, drag, lift, iters, inflow_scale);
  }
  return hipGetLastError();
}

}  // namespace mdq
