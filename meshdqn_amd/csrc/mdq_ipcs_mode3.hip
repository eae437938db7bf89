// IPCS: the three-kernel LDS-atomic operator mode (mode 3): at_velocity_kernel, at_pressure_kernel, at_correction_kernel
// and their helpers.  Included by mdq_ipcs.hip (the entry unit) only, behind its own two kernels.
#ifndef MDQ_CORR_MX0_INTERLEAVE
#define MDQ_CORR_MX0_INTERLEAVE false
#endif
#ifndef MDQ_PCG_REGM
#define MDQ_PCG_REGM 1
#endif
namespace mdq {

// float kept in a register -> double at the point of use: the asm stops the compiler from hoisting the conversion
// out of the Krylov loop, which turns 4-byte loop invariants into 8-byte ones (measured: they were then spilled to
// scratch and re-read one by one in every vector phase of every iteration)
__device__ __forceinline__ double f2d(float f) {
  asm volatile("" : "+v"(f));
  return (double)f;
}

// ================================================================== matrix-free kernel, LDS-atomic accumulation (mode 3)
//
// Same element operators as mode 2, but the element results are accumulated straight into an LDS
// result vector with hardware LDS fp64 atomics (ds_add_f64) instead of going through a tile and an
// ordered row gather.  That frees the 96 KB tile: the search direction p, the residual r (= s) AND
// the result vector all live in LDS, only v stays in registers, so the element phase can interleave
// several triangles per thread (FP64 ILP) without register spills, with two barriers per operator
// application.  Price: the summation order of the <= 8 contributions per row depends on timing, so
// results are reproducible to round-off only (modes 0-2 are bitwise reproducible).

constexpr int AT_PAIR = 2;  // triangles interleaved per thread per round

template <int TPAIR = AT_PAIR>
struct AtMetaT {
  int w[TPAIR][6];
  Geo g[TPAIR];
};
using AtMeta = AtMetaT<AT_PAIR>;

template <int TW = WG, int TPAIR = AT_PAIR>
__device__ __forceinline__ void at_prefetch(const EnvView& v, AtMetaT<TPAIR>& m, int round) {
#pragma unroll
  for (int j = 0; j < TPAIR; ++j) {
    const int e = threadIdx.x + (round * TPAIR + j) * TW;
    if (e < v.nt) {
#pragma unroll
      for (int i = 0; i < 6; ++i) m.w[j][i] = v.mf_scat[i * v.NT + e];
      m.g[j] = load_geo(v, e);
    }
  }
}

// Y[dof] += element results for every triangle (Y zeroed and published by the caller).
// op(e, geo, dofs, outflow_edge, ye).  On entry m holds round 0; on exit again (rolling prefetch).
// INTERLEAVE = true computes the AT_PAIR triangles of a round side by side (FP64 ILP for the hot
// operator applications); false runs them one after the other (register-hungry right-hand sides).
template <bool INTERLEAVE, int TW = WG, int TPAIR = AT_PAIR, class ElemOp>
__device__ __forceinline__ void atomic_accumulate(const EnvView& v, double* Yd, AtMetaT<TPAIR>& m, ElemOp op) {
  const int nrounds = (v.nt + TPAIR * TW - 1) / (TPAIR * TW);
  // (delaying the odd waves by 256-1536 cycles to de-phase LDS and FP64 phases only added the delay: measured)
  for (int round = 0; round < nrounds; ++round) {
    if (INTERLEAVE) {
      double2 ye[TPAIR][6];
      int dof[TPAIR][6];
#pragma unroll
      for (int j = 0; j < TPAIR; ++j) {
        const int e = threadIdx.x + (round * TPAIR + j) * TW;
        if (e < v.nt) {
          ElemIdx E;
#pragma unroll
          for (int i = 0; i < 6; ++i) E.dof[i] = dof[j][i] = m.w[j][i] & 0xFFF;
          op(e, m.g[j], E, ((m.w[j][0] >> 28) & 3) - 1, ye[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < TPAIR; ++j) {
        const int e = threadIdx.x + (round * TPAIR + j) * TW;
        if (e < v.nt) {
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            unsafeAtomicAdd(Yd + 2 * dof[j][i], ye[j][i].x);
            unsafeAtomicAdd(Yd + 2 * dof[j][i] + 1, ye[j][i].y);
          }
        }
      }
    } else {
#pragma unroll 1
      for (int j = 0; j < TPAIR; ++j) {
        const int e = threadIdx.x + (round * TPAIR + j) * TW;
        if (e < v.nt) {
          ElemIdx E;
          double2 ye[6];
          // (explicit selects: a runtime index into the register arrays would demote them to scratch)
          const int* wj = (TPAIR == 1 || j == 0) ? m.w[0] : m.w[TPAIR - 1];
          const Geo gj = (TPAIR == 1 || j == 0) ? m.g[0] : m.g[TPAIR - 1];
#pragma unroll
          for (int i = 0; i < 6; ++i) E.dof[i] = wj[i] & 0xFFF;
          op(e, gj, E, ((wj[0] >> 28) & 3) - 1, ye);
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            unsafeAtomicAdd(Yd + 2 * E.dof[i], ye[i].x);
            unsafeAtomicAdd(Yd + 2 * E.dof[i] + 1, ye[i].y);
          }
        }
      }
    }
    at_prefetch<TW, TPAIR>(v, m, round + 1 < nrounds ? round + 1 : 0);
  }
}

// The outflow-facet term, one ENTRY per thread (18 entries per outflow facet, a few hundred per mesh): every
// thread adds coef * B_entry x[col] to Y[row] with LDS atomics, between the barrier that publishes the zeroed Y
// and the element loop, so that the term costs one global-load latency of the waves that own entries instead of a
// serial per-row chain of them between two barriers.  (row, col) of entry `tid` is found once per launch from the
// element slot list (bo_src = cell * 36 + i * 6 + j) and kept packed in one register; entries beyond the
// workgroup size (more than 28 / 42 outflow facets; not on the training meshes) are looked up on the fly.  No thread owns
// outflow rows: any number of them may share a residue modulo the workgroup size.
struct BoEnt {
  int rc;   // row << 12 | col of entry threadIdx.x, -1 if none
  int nbe;  // entries of this environment
};
__device__ __forceinline__ int outflow_entry_rc(const EnvView& v, int t) {
  const int slot = v.bo_src[t];
  const int e = slot / 36, ij = slot - e * 36, i = ij / 6, j = ij - i * 6;
  return ((v.mf_scat[i * v.NT + e] & 0xFFF) << 12) | (v.mf_scat[j * v.NT + e] & 0xFFF);
}
__device__ __forceinline__ BoEnt outflow_entries_owned(const EnvView& v) {
  BoEnt o;
  o.nbe = v.nbo > 0 ? v.bo_ptr[v.nbo] : 0;
  o.rc = (int)threadIdx.x < o.nbe ? outflow_entry_rc(v, threadIdx.x) : -1;
  return o;
}
__device__ __forceinline__ void outflow_entry_apply(const EnvView& v, int t, int rc, double coef, const double2* x,
                                                    double* Yd) {
  const double4 bv = reinterpret_cast<const double4*>(v.bo_val)[t];
  const double2 xc = x[rc & 0xFFF];
  const int row = rc >> 12;
  unsafeAtomicAdd(Yd + 2 * row, coef * (bv.x * xc.x + bv.y * xc.y));
  unsafeAtomicAdd(Yd + 2 * row + 1, coef * (bv.z * xc.x + bv.w * xc.y));
}
template <int TW>
__device__ __forceinline__ void outflow_entries_add(const EnvView& v, const BoEnt& o, double coef, const double2* x,
                                                    double* Yd) {
  if (o.rc >= 0) outflow_entry_apply(v, threadIdx.x, o.rc, coef, x, Yd);
  for (int t = threadIdx.x + TW; t < o.nbe; t += TW) outflow_entry_apply(v, t, outflow_entry_rc(v, t), coef, x, Yd);
}


// ---- mode 3 as three kernels per time step (separate register allocation per phase: the BiCGStab
// loop then runs without spill reloads; state is handed over through global memory as before) ----
template <int TW, int TROWS, int TPAIR>
__global__ __launch_bounds__(TW) void at_velocity_kernel(mdq_ipcs_desc d, int32_t* iters, const double* inflow_scale, int nsteps,
                                                         int step, int fresh) {
  extern __shared__ __align__(16) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const EnvView v = env_view(d, b);
  const double ai = inflow_factor(inflow_scale, b, nsteps, step);
  const int n2 = v.n2, nv = v.nv;
  const LdsPlan P = lds_plan(d.N2, d.NV, d.NSE1);
  const double a = uniform_double(v.rho / v.dt), mu = v.mu;
  (void)a; (void)mu; (void)nv; (void)n2;
  double* red = smem;  // 64 doubles
  double* U = smem + 64;
  double* w = v.work;
  double2* xs = reinterpret_cast<double2*>(w + 12 * (int64_t)d.NT);  // x of the velocity solve = u*
  double* pnew = reinterpret_cast<double*>(xs + 6 * (int64_t)d.N2);
  int rsel = 0;  // parity of the one-barrier reductions
  (void)rsel; (void)pnew; (void)red;
  double2* Pl = reinterpret_cast<double2*>(U);  // search direction p / staged operator input
  double2* Rl = Pl + P.N2p;                      // residual r (= s)
  double2* Yl = Rl + P.N2p;                      // operator result (atomic accumulation)
  double* Yd = reinterpret_cast<double*>(Yl);
  AtMetaT<TPAIR> tm;
  at_prefetch<TW, TPAIR>(v, tm, 0);
  const BoEnt bo_ent = outflow_entries_owned(v);
  int it_u = 0;
  double2* hist = xs + d.N2;                                          // u* of the step before the last
  double2* hist2 = xs + 2 * (int64_t)d.N2;                            // and of the one before that
  double2* hist3 = xs + 4 * (int64_t)d.N2;                            // and one more (slot 3 holds the counter)
  double2* hist4 = xs + 5 * (int64_t)d.N2;
  double* histc = reinterpret_cast<double*>(xs + 3 * (int64_t)d.N2);  // [0]: tentative velocities stored so far
  // `fresh` (all three kernels, step 0 of mdq_ipcs_evolve_fresh): a new mesh - the stored history counts as empty and the
  // iteration words are assigned, what a reset_history_kernel launch in front of this one would have left
  const int nhist = (fresh && step == 0) ? 0 : (int)histc[0];
#ifdef MDQ_AT_TRACE
  long long tq_ = __builtin_amdgcn_s_memtime();
#endif
  __syncthreads();
  AT_STAMP(0)
  {
    // ================= step 1: tentative velocity
    // Row loops: thread `tid` owns rows tid + k * TW.  All reads use the clamped row (rows past n2 re-read row
    // n2 - 1, value unused) and come first, so that the TROWS loads of a phase are in flight together instead of
    // one conditional block (and one LDS / L2 round trip) per row; only the writes are predicated.
    int rc[TROWS];
    float2 idg[TROWS];
    unsigned flm = 0;  // bit k: row k of this thread carries a Dirichlet value
#pragma unroll
    for (int k = 0; k < TROWS; ++k) rc[k] = min(tid + k * TW, n2 - 1);
    {
      // u_n and p_n staged in LDS (p and r are free until the solve starts): the right-hand-side element loop
      // gathers 6 + 3 values per triangle from LDS instead of from L2
      double2 un_[TROWS], dg_[TROWS];
      unsigned char fl_[TROWS];
#pragma unroll
      for (int k = 0; k < TROWS; ++k) {
        un_[k] = v.u_n[rc[k]];
        dg_[k] = v.idiag1[rc[k]];
        fl_[k] = v.bcu_flag[rc[k]];
      }
      double* Pn = reinterpret_cast<double*>(Rl);
      for (int i = tid; i < nv; i += TW) Pn[i] = v.p_n[i];
#pragma unroll
      for (int k = 0; k < TROWS; ++k) {
        const int row = tid + k * TW;
        idg[k] = (row < n2 && !fl_[k]) ? make_float2((float)dg_[k].x, (float)dg_[k].y) : make_float2(0.f, 0.f);
        flm |= fl_[k] ? 1u << k : 0u;
        if (row < n2) {
          Pl[row] = un_[k];
          Yl[row] = make_double2(0.0, 0.0);
        }
      }
    }
    __syncthreads();
    outflow_entries_add<TW>(v, bo_ent, 0.5 * mu, Pl, Yd);  // + mu/2 <nabla_grad(u_n) n, v> on the outflow rows
    {
      const double* Pn = reinterpret_cast<const double*>(Rl);
      atomic_accumulate<false, TW, TPAIR>(v, Yd, tm, [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
        double2 ue[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) ue[i] = Pl[E.dof[i]];
        double pe[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) pe[i] = Pn[E.dof[i]];
        elem_rhs1_vol(g, a, mu, v.rho, ue, pe, ye);
      });
    }
    // initial guess: polynomial extrapolation in time of the previous tentative velocities (xs still holds
    // u*_n, hist.. hist4 the four before it), up to quartic as the history fills; u_n while there is none.
    // dt is far below the flow's time scales, so every order removes about two digits of initial residual
    // (11 BiCGStab iterations without, 8 linear, 6 quadratic, 3 cubic, 2.6 quartic; beyond that the 1e-10
    // solver noise of the history, amplified by the coefficients, is the floor).  Dirichlet values hold.
    // The history loads are issued here, in front of the barrier that ends the element loop.
    double2 x0[TROWS];
    {
      // binomial coefficients of the order in use: x0 = c1 u*_n + c2 u*_{n-1} + ... (alternating signs)
      const double c1 = nhist >= 5 ? 5.0 : nhist == 4 ? 4.0 : nhist == 3 ? 3.0 : 2.0;
      const double c2 = nhist >= 5 ? -10.0 : nhist == 4 ? -6.0 : nhist == 3 ? -3.0 : -1.0;
      const double c3 = nhist >= 5 ? 10.0 : nhist == 4 ? 4.0 : 1.0;
      const double c4 = nhist >= 5 ? -5.0 : -1.0;
      double2 us1[TROWS];
#pragma unroll
      for (int k = 0; k < TROWS; ++k) us1[k] = xs[rc[k]];
      if (nhist >= 2) {
        double2 h[TROWS];
#pragma unroll
        for (int k = 0; k < TROWS; ++k) h[k] = hist[rc[k]];
#pragma unroll
        for (int k = 0; k < TROWS; ++k) x0[k] = make_double2(c1 * us1[k].x + c2 * h[k].x, c1 * us1[k].y + c2 * h[k].y);
        if (nhist >= 3) {
          double2 h2[TROWS];
#pragma unroll
          for (int k = 0; k < TROWS; ++k) h2[k] = hist2[rc[k]];
#pragma unroll
          for (int k = 0; k < TROWS; ++k) x0[k] = make_double2(x0[k].x + c3 * h2[k].x, x0[k].y + c3 * h2[k].y);
          if (nhist >= 4) {
            double2 h3[TROWS];
#pragma unroll
            for (int k = 0; k < TROWS; ++k) h3[k] = hist3[rc[k]];
#pragma unroll
            for (int k = 0; k < TROWS; ++k) x0[k] = make_double2(x0[k].x + c4 * h3[k].x, x0[k].y + c4 * h3[k].y);
            if (nhist >= 5) {
#pragma unroll
              for (int k = 0; k < TROWS; ++k) {
                const double2 h4 = hist4[rc[k]];
                x0[k] = make_double2(x0[k].x + h4.x, x0[k].y + h4.y);
              }
            }
#pragma unroll
            for (int k = 0; k < TROWS; ++k)
              if (tid + k * TW < n2) hist4[tid + k * TW] = h3[k];
          }
#pragma unroll
          for (int k = 0; k < TROWS; ++k)
            if (tid + k * TW < n2) hist3[tid + k * TW] = h2[k];
        }
#pragma unroll
        for (int k = 0; k < TROWS; ++k)
          if (tid + k * TW < n2) hist2[tid + k * TW] = h[k];
      } else {
#pragma unroll
        for (int k = 0; k < TROWS; ++k) x0[k] = v.u_n[rc[k]];
      }
#pragma unroll
      for (int k = 0; k < TROWS; ++k)
        if (tid + k * TW < n2) hist[tid + k * TW] = us1[k];
    }
    double2 lf[TROWS];
    double gx[TROWS];
#pragma unroll
    for (int k = 0; k < TROWS; ++k) {
      lf[k] = scaled2(ai, v.lift1[rc[k]]);
      gx[k] = ai * v.bcu_gx[rc[k]];
    }
    __syncthreads();
    AT_STAMP(1)
    double acc[2] = {0.0, 0.0};
    double2 f[TROWS];
#pragma unroll
    for (int k = 0; k < TROWS; ++k) f[k] = Yl[rc[k]];
#pragma unroll
    for (int k = 0; k < TROWS; ++k) {
      const int row = tid + k * TW;
      const bool fl = (flm >> k) & 1u;
      const double2 g = make_double2(gx[k], 0.0);
      if (fl) x0[k] = g;
      if (row < n2) {
        Yl[row] = make_double2(0.0, 0.0);
        xs[row] = x0[k];
        Pl[row] = x0[k];
        const double2 bi = fl ? g : make_double2((f[k].x - lf[k].x) * f2d(idg[k].x), (f[k].y - lf[k].y) * f2d(idg[k].y));
        acc[0] += bi.x * bi.x + bi.y * bi.y;
      }
    }
    __syncthreads();
    AT_STAMP(2)
    outflow_entries_add<TW>(v, bo_ent, -0.5 * mu, Pl, Yd);
    atomic_accumulate<(TPAIR > 1), TW, TPAIR>(v, Yd, tm, [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
      double2 xe[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) xe[i] = Pl[E.dof[i]];
      elem_velocity(g, a, mu, xe, ye);
    });
    __syncthreads();
    AT_STAMP(3)
    double2 vv[TROWS];
#pragma unroll
    for (int k = 0; k < TROWS; ++k) {
      const int row = tid + k * TW;
      vv[k] = make_double2(0.0, 0.0);
      if (row < n2) {
        const double2 ax = Yl[row];
        // r0 = D^-1 (f - A_full x0) on free rows, 0 on constrained rows (idg = 0 there)
        const double2 r0 = make_double2((f[k].x - ax.x) * f2d(idg[k].x), (f[k].y - ax.y) * f2d(idg[k].y));
        Rl[row] = r0;
        acc[1] += r0.x * r0.x + r0.y * r0.y;
      }
    }
    block_sum<2, TW / 64>(acc, red);
    // p = 0 (only now: the outflow rows above still gathered x0 from Pl until the barriers of the reduction)
#pragma unroll
    for (int k = 0; k < TROWS; ++k) {
      const int row = tid + k * TW;
      if (row < n2) Pl[row] = make_double2(0.0, 0.0);
    }
    {
      const double bb = acc[0], tol2 = uniform_double(d.rtol * d.rtol * bb);
      double rr = acc[1];
      if (rr > tol2 && bb != 0.0) {
        double rho = rr, rho_old = 1.0, alpha = 1.0, omega = 1.0;
        int it = 0;
        // shadow residual in registers (own rows).  BiCGStab accepts ANY fixed shadow vector with
        // (rh, r0) != 0; we take r0 rounded to fp32, which halves its register footprint.
        float2 rh[TROWS];
        {
          double a0[1] = {0.0};
#pragma unroll
          for (int k = 0; k < TROWS; ++k) {
            const int row = tid + k * TW;
            rh[k] = make_float2(0.f, 0.f);
            if (row < n2) {
              const double2 r0 = Rl[row];
              rh[k] = make_float2((float)r0.x, (float)r0.y);
              a0[0] += (double)rh[k].x * r0.x + (double)rh[k].y * r0.y;
            }
          }
          block_sum1<1, TW / 64>(a0, red, rsel);
          rho = a0[0];  // (rh, r0)
        }
        AT_STAMP(4)
        while (it < d.maxit_u) {
          ++it;
          const double beta = (rho / rho_old) * (alpha / omega);
#pragma unroll
          for (int k = 0; k < TROWS; ++k) {
            const int row = tid + k * TW;
            if (row < n2) {
              const double2 ri = Rl[row], pi = Pl[row];
              Pl[row] = make_double2(ri.x + beta * (pi.x - omega * vv[k].x), ri.y + beta * (pi.y - omega * vv[k].y));
              Yl[row] = make_double2(0.0, 0.0);
            }
          }
          __syncthreads();
          AT_STAMP(5)
          outflow_entries_add<TW>(v, bo_ent, -0.5 * mu, Pl, Yd);
          atomic_accumulate<(TPAIR > 1), TW, TPAIR>(v, Yd, tm, [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
            double2 xe[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) xe[i] = Pl[E.dof[i]];
            elem_velocity(g, a, mu, xe, ye);
          });
          __syncthreads();
          AT_STAMP(6)
          double a1[1] = {0.0};
#pragma unroll
          for (int k = 0; k < TROWS; ++k) {
            const int row = tid + k * TW;
            if (row < n2) {
              const double2 yv = Yl[row];
              vv[k] = make_double2(yv.x * f2d(idg[k].x), yv.y * f2d(idg[k].y));
              a1[0] += f2d(rh[k].x) * vv[k].x + f2d(rh[k].y) * vv[k].y;
            }
          }
          block_sum1<1, TW / 64>(a1, red, rsel);
          AT_STAMP(7)
          if (a1[0] == 0.0) break;
          alpha = rho / a1[0];
          // s = r - alpha v ; no early exit on |s| (saves a reduction; the check on |r| follows)
#pragma unroll
          for (int k = 0; k < TROWS; ++k) {
            const int row = tid + k * TW;
            if (row < n2) {
              const double2 ri = Rl[row];
              Rl[row] = make_double2(ri.x - alpha * vv[k].x, ri.y - alpha * vv[k].y);
              Yl[row] = make_double2(0.0, 0.0);
            }
          }
          __syncthreads();  // publish s and the zeroed result vector
          AT_STAMP(8)
          outflow_entries_add<TW>(v, bo_ent, -0.5 * mu, Rl, Yd);
          atomic_accumulate<(TPAIR > 1), TW, TPAIR>(v, Yd, tm, [&](int e, const Geo& g, const ElemIdx& E, int ko, double2(&ye)[6]) {
            double2 xe[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) xe[i] = Rl[E.dof[i]];
            elem_velocity(g, a, mu, xe, ye);
          });
          // x of the own rows: issue the global reads now, they are consumed after the reduction
          double2 xo[TROWS];
#pragma unroll
          for (int k = 0; k < TROWS; ++k) {
            const int row = tid + k * TW;
            xo[k] = row < n2 ? xs[row] : make_double2(0.0, 0.0);
          }
          __syncthreads();
          AT_STAMP(9)
          double a3[2] = {0.0, 0.0};
          double2 t[TROWS];
#pragma unroll
          for (int k = 0; k < TROWS; ++k) {
            const int row = tid + k * TW;
            t[k] = make_double2(0.0, 0.0);
            if (row < n2) {
              const double2 yv = Yl[row], sv = Rl[row];
              t[k] = make_double2(yv.x * f2d(idg[k].x), yv.y * f2d(idg[k].y));
              a3[0] += t[k].x * sv.x + t[k].y * sv.y;
              a3[1] += t[k].x * t[k].x + t[k].y * t[k].y;
            }
          }
          block_sum1<2, TW / 64>(a3, red, rsel);
          AT_STAMP(10)
          if (a3[1] == 0.0) break;
          omega = a3[0] / a3[1];
          double a4[2] = {0.0, 0.0};
#pragma unroll
          for (int k = 0; k < TROWS; ++k) {
            const int row = tid + k * TW;
            if (row < n2) {
              const double2 pi = Pl[row], sv = Rl[row];
              xs[row] = make_double2(xo[k].x + alpha * pi.x + omega * sv.x, xo[k].y + alpha * pi.y + omega * sv.y);
              const double2 rn = make_double2(sv.x - omega * t[k].x, sv.y - omega * t[k].y);
              Rl[row] = rn;
              a4[0] += rn.x * rn.x + rn.y * rn.y;
              a4[1] += f2d(rh[k].x) * rn.x + f2d(rh[k].y) * rn.y;
            }
          }
          block_sum1<2, TW / 64>(a4, red, rsel);
          AT_STAMP(11)
          rr = a4[0];
          if (!(rr > tol2)) break;
          rho_old = rho;
          rho = a4[1];
          if (rho == 0.0 || omega == 0.0) break;
        }
        it_u += it;
      }
    }
    __syncthreads();  // xs (= u*) complete: the element loops of steps 2 and 3 gather it
    AT_STAMP(12)
  }
  if (tid == 0) {
    histc[0] = (double)(nhist < 5 ? nhist + 1 : 5);
    if (iters) iters[3 * b + 0] = ((fresh && step == 0) ? 0 : iters[3 * b + 0]) + it_u;
  }
}

// NTH = 1024 for the direct solver (its dense phases are latency-bound streams of 0.8 MB of factors: twice the loads
// in flight per CU); the CG variant keeps the 512-thread shape its reductions are written for.
template <bool K1_LDS, int NTH = WG>
__global__ __launch_bounds__(NTH) void at_pressure_kernel(mdq_ipcs_desc d, int32_t* iters, int fresh) {
  extern __shared__ __align__(16) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  // (`fresh`: the first step of mdq_ipcs_evolve_fresh - the iteration word starts from zero; cleared HERE by the thread that
  //  adds to it at the end, so that the flag is not live across the solve: this kernel sits at its register cap)
  if (fresh && tid == 0 && iters) iters[3 * b + 1] = 0;
  const EnvView v = env_view(d, b);
  const int n2 = v.n2, nv = v.nv;
  const LdsPlan P = lds_plan(d.N2, d.NV, d.NSE1);
  const double a = v.rho / v.dt, mu = v.mu;
  (void)a; (void)mu; (void)nv; (void)n2;
  double* red = smem;  // 64 doubles
  double* U = smem + 64;
  double* w = v.work;
  double2* xs = reinterpret_cast<double2*>(w + 12 * (int64_t)d.NT);  // x of the velocity solve = u*
  double* pnew = reinterpret_cast<double*>(xs + 6 * (int64_t)d.N2);
  int rsel = 0;  // parity of the one-barrier reductions
  (void)rsel; (void)pnew; (void)red;
  double* px = U;
  double* pr = px + P.NVp;
  double* pp = pr + P.NVp;
  double* pq = pp + P.NVp;
  double* lK = pq + P.NVp;
  int32_t* lci = reinterpret_cast<int32_t*>(lK + d.NSE1);
  int32_t* lso = lci + d.NSE1 + (d.NSE1 & 1);
  double* escr1 = w;
  const int nsl1 = (nv + 63) >> 6;
  const int32_t* so1 = K1_LDS ? lso : v.sl1_off;
  const int32_t* ci1 = K1_LDS ? lci : v.sl1_col;
  const double* K1 = K1_LDS ? lK : v.K1s;
  int it_p = 0;
#ifdef MDQ_AT_TRACE
  const long long tq0_ = __builtin_amdgcn_s_memtime();
#endif
  {
    // ================= step 2: pressure
    if (K1_LDS && !d.pd_enabled) {
      const int ne1 = v.sl1_off[nsl1];
      for (int kk = tid; kk < ne1; kk += NTH) {
        lK[kk] = v.K1s[kk];
        lci[kk] = v.sl1_col[kk];
      }
      for (int kk = tid; kk <= nsl1; kk += NTH) lso[kk] = v.sl1_off[kk];
    }
    (void)escr1;
    for (int i = tid; i < nv; i += NTH) pr[i] = 0.0;
    __syncthreads();
    rhs2_accumulate_lds<NTH>(v, d, xs, v.p_n, pr);
    // own-row data of the scaling, loaded in front of the barrier that ends the accumulation
    constexpr int PRW = 2048 / NTH;   // own rows per thread held in registers (vertex capacity of the LDS modes < 2048)
    double sd_[PRW], pn_[PRW];
    unsigned fl_ = 0;
#pragma unroll
    for (int k = 0; k < PRW; ++k) {
      const int i = min(tid + k * NTH, nv - 1);
      sd_[k] = v.sdiagK[i];
      pn_[k] = v.p_n[i];
      fl_ |= v.bcp_flag[i] ? 1u << k : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PRW; ++k) {
      const int i = tid + k * NTH;
      if (i < nv) {
        pr[i] = ((fl_ >> k) & 1u) ? 0.0 : pr[i] / sd_[k];
        px[i] = pn_[k] * sd_[k];
      }
    }
    for (int i = tid + PRW * NTH; i < nv; i += NTH) {   // (nv beyond 2048: generic tail)
      const double sd = v.sdiagK[i];
      pr[i] = v.bcp_flag[i] ? 0.0 : pr[i] / sd;
      px[i] = v.p_n[i] * sd;
    }
    // (an environment whose factors could not be built on the device - mdq_ipcs_factorize_pressure, header nparts = 0 -
    // falls back to the Krylov solve)
    if (d.pd_enabled && d.pd_hdr[4 * (int64_t)b + 2] > 0) {
      const PdView pd = pd_view(d, b);
#ifdef MDQ_AT_TRACE
      { const long long tn_ = __builtin_amdgcn_s_memtime(); if (tid == 0 && b == 0) mdq_pt_trace_buf[0] += tn_ - tq0_; }
#endif
      pressure_direct<NTH>(pd, nv, pr, px, pp, pq, lK);
    } else {
      int itc = -1;
      // (the 1024-thread instance is the direct solver's shape - 128 VGPRs per thread: the register-hungry Krylov variants
      //  compiled into it cost 272 B of scratch per lane in round 3 without ever running there; an environment without
      //  factors takes the plain register CG below)
      if constexpr (NTH <= 512) {
        if (d.pcg_degree < 0)                    // two-level additive preconditioner (geometric aggregates)
          itc = cg_pressure_2l<NTH>(nv, so1, ci1, K1, v.coords, d.rtol, d.maxit_p, px, pr, pp, P.NVp, red, rsel);
        else if (nv <= 2 * NTH && d.pcg_degree > 0)   // rows in registers, Chebyshev-preconditioned (degree 1: Jacobi only)
          itc = cg_pressure_cheb<NTH>(nv, so1, ci1, K1, d.rtol, d.maxit_p, d.pcg_degree, px, pr, pp, red, rsel);
        if (itc < 0 && nv <= 2 * NTH && d.pcg_degree == 0 && MDQ_PCG_REGM)   // rows in registers, branch-free application
          itc = cg_pressure_regm<NTH>(nv, so1, ci1, K1, d.rtol, d.maxit_p, px, pr, pp, red, rsel);
      }
      if (itc >= 0)
        it_p += itc;
      else if (nv <= 2 * NTH)
        it_p += cg_pressure_reg<NTH>(nv, so1, ci1, K1, d.rtol, d.maxit_p, px, pr, pp, red, rsel);
      else
        it_p += cg_pressure(nv, so1, ci1, K1, d.rtol, d.maxit_p, px, pr, pp, pq, red);
    }
    for (int i = tid; i < nv; i += NTH) pnew[i] = px[i] / v.sdiagK[i];
    __syncthreads();

  }
  if (tid == 0 && iters) iters[3 * b + 1] += it_p;
}

static __global__ __launch_bounds__(WG) void at_correction_kernel(mdq_ipcs_desc d, int nsteps, int step, double* drag,
                                                            double* lift, int32_t* iters, const double* inflow_scale,
                                                            int fresh) {
  extern __shared__ __align__(16) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const EnvView v = env_view(d, b);
  const double ai = inflow_factor(inflow_scale, b, nsteps, step);
  const bool fresh0 = fresh && step == 0;
  const int n2 = v.n2, nv = v.nv;
  const LdsPlan P = lds_plan(d.N2, d.NV, d.NSE1);
  const double a = v.rho / v.dt, mu = v.mu;
  (void)a; (void)mu; (void)nv; (void)n2;
  double* red = smem;  // 64 doubles
  double* U = smem + 64;
  double* w = v.work;
  double2* xs = reinterpret_cast<double2*>(w + 12 * (int64_t)d.NT);  // x of the velocity solve = u*
  double* pnew = reinterpret_cast<double*>(xs + 6 * (int64_t)d.N2);
  int rsel = 0;  // parity of the one-barrier reductions
  (void)rsel; (void)pnew; (void)red;
  double2* Pl = reinterpret_cast<double2*>(U);
  double2* Yl = Pl + P.N2p;
  double* Yd = reinterpret_cast<double*>(Yl);
  AtMeta tm;
  at_prefetch(v, tm, 0);
  int it_m = 0;
  // ring of the last three corrections u_{n+1} - u* (in the slab region the assembled modes use for their history)
  double2* cring = reinterpret_cast<double2*>(w + work_hist_offset(d.NV, d.NT, d.NE));
  double* ccnt = reinterpret_cast<double*>(cring + 3 * (int64_t)d.N2);  // [0]: corrections stored, [1]: ring position
  const int nc = fresh0 ? 0 : (int)ccnt[0], rp = fresh0 ? 0 : (int)ccnt[1];
#ifdef MDQ_AT_TRACE
  long long tq_ = __builtin_amdgcn_s_memtime();
#endif
  __syncthreads();
  CT_STAMP(0)
  {
    // ================= step 3: velocity correction (mass solve, both components)
    double2 x[MF_ROWS], r[MF_ROWS], p[MF_ROWS];
    double ism[MF_ROWS];
    double am[2] = {0.0, 0.0};
    // Row loops as in at_velocity_kernel: clamped rows, all loads of a phase issued before their first use.
    int rc[MF_ROWS];
#pragma unroll
    for (int k = 0; k < MF_ROWS; ++k) rc[k] = min(tid + k * WG, n2 - 1);
    double* Dp = reinterpret_cast<double*>(Yl + P.N2p);   // [nv] pressure increment, staged for the element loop
    // initial guess of the correction: extrapolation in time of the stored ones (constant, linear, quadratic as the
    // ring fills): 5.0 CG iterations per step with the previous correction alone, 1.7 with the quadratic guess (the
    // velocity solve then needs 2.9 instead of 2.6 iterations: u_n now carries the full 1e-10 solver noise).
    // Dirichlet rows keep u* = g (their stored corrections are 0).
    auto load_delta = [&](double2(&dl)[MF_ROWS]) {
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) dl[k] = make_double2(0.0, 0.0);
      if (nc >= 1) {
        const double2* c1 = cring + (int64_t)((rp + 2) % 3) * d.N2;   // newest
        const double2* c2 = cring + (int64_t)((rp + 1) % 3) * d.N2;
        const double2* c3 = cring + (int64_t)rp * d.N2;               // oldest (overwritten at the end of this launch)
#pragma unroll
        for (int k = 0; k < MF_ROWS; ++k) dl[k] = c1[rc[k]];
        if (nc >= 2) {
          const double w1 = nc >= 3 ? 3.0 : 2.0, w2 = nc >= 3 ? -3.0 : -1.0;
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const double2 b2 = c2[rc[k]];
            dl[k] = make_double2(w1 * dl[k].x + w2 * b2.x, w1 * dl[k].y + w2 * b2.y);
          }
          if (nc >= 3) {
#pragma unroll
            for (int k = 0; k < MF_ROWS; ++k) {
              const double2 b3 = c3[rc[k]];
              dl[k] = make_double2(dl[k].x + b3.x, dl[k].y + b3.y);
            }
          }
        }
      }
    };
    // FUSED start (15 of 16 steps once the ring is full): with x0 = u* + delta0 the initial residual is
    //   f3 - M x0 = (M u* - g) - M (u* + delta0) = -g - M delta0,
    // ONE element loop (the right-hand-side operator applied to -delta0) instead of two (f3, then M x0), and no
    // lifting vector (delta0 vanishes on the Dirichlet rows).  What it cannot give is |b| of the stopping test
    // rtol |b|, which needs f3 itself: the value of the last exact start is used (it changes by < 1e-3 per step);
    // every 16th step, and while the ring fills, the exact two-loop start runs and refreshes it.
    const double bb_lag = fresh0 ? 0.0 : ccnt[2];
    const int cstep = fresh0 ? 0 : (int)ccnt[3];
    const bool fused = nc >= 3 && bb_lag > 0.0 && (cstep & 15) != 0;
    {
      // operator input (u*, or -delta0) and p_new - p_n staged in LDS: the element loop gathers from LDS, not L2
      double2 us[MF_ROWS];
      if (!fused) {
#pragma unroll
        for (int k = 0; k < MF_ROWS; ++k) us[k] = xs[rc[k]];
      } else {
        load_delta(us);
#pragma unroll
        for (int k = 0; k < MF_ROWS; ++k) us[k] = make_double2(-us[k].x, -us[k].y);
      }
      for (int i = tid; i < nv; i += WG) Dp[i] = pnew[i] - v.p_n[i];
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        if (row < n2) {
          Pl[row] = us[k];
          Yl[row] = make_double2(0.0, 0.0);
        }
      }
    }
    __syncthreads();
    atomic_accumulate<true>(v, Yd, tm, [&](int, const Geo& g, const ElemIdx& E, int, double2(&ye)[6]) {
      double2 ue[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) ue[i] = Pl[E.dof[i]];
      double dp[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) dp[i] = Dp[E.dof[i]];
      elem_rhs3(g, v.dt, ue, dp, ye);
    });
    // own rows of the global vectors of the next phase: issued in front of the barrier that ends the element loop
    double2 l3[MF_ROWS], dlt[MF_ROWS];
    unsigned flm = 0;
    if (!fused) load_delta(dlt);   // (the fused start reads delta0 back from its LDS copy below)
#pragma unroll
    for (int k = 0; k < MF_ROWS; ++k) {
      // fused start: u* of the own rows (the LDS copy holds -delta0; its Dirichlet rows carry this step's a g from step 1)
      l3[k] = fused ? xs[rc[k]] : scaled2(ai, v.lift3[rc[k]]);
      ism[k] = v.sdiagM[rc[k]];
      flm |= v.bcu_flag[rc[k]] ? 1u << k : 0u;
    }
    __syncthreads();
    CT_STAMP(1)
    double bb;
    if (fused) {
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        r[k] = Yl[rc[k]];
        const double2 md = Pl[rc[k]];
        dlt[k] = make_double2(-md.x, -md.y);
      }
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        const bool fl = (flm >> k) & 1u;
        ism[k] = (row < n2 && !fl) ? 1.0 / ism[k] : 0.0;
        r[k] = make_double2(r[k].x * ism[k], r[k].y * ism[k]);          // 0 on constrained rows and past n2
        p[k] = r[k];
        am[1] += r[k].x * r[k].x + r[k].y * r[k].y;
        // scaled unknown S x0 on the free rows, u* = g on the Dirichlet rows
        x[k] = fl ? l3[k] : make_double2((l3[k].x + dlt[k].x) / (ism[k] != 0.0 ? ism[k] : 1.0),
                                          (l3[k].y + dlt[k].y) / (ism[k] != 0.0 ? ism[k] : 1.0));
        if (row >= n2) x[k] = make_double2(0.0, 0.0);
      }
      double a1r[1] = {am[1]};
      block_sum<1>(a1r, red);
      am[1] = a1r[0];
      bb = bb_lag;
      CT_STAMP(2)
      CT_STAMP(3)
    } else {
      double2 f3[MF_ROWS];
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        f3[k] = Yl[rc[k]];
        x[k] = Pl[rc[k]];      // u* (own row)
      }
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        const bool fl = (flm >> k) & 1u;
        ism[k] = (row < n2 && !fl) ? 1.0 / ism[k] : 0.0;
        if (!fl) x[k] = make_double2(x[k].x + dlt[k].x, x[k].y + dlt[k].y);
        if (row < n2) {
          Yl[row] = make_double2(0.0, 0.0);
          Pl[row] = x[k];      // stage S^-1 (S x0) = x0
          const double2 bi = fl ? x[k] : make_double2((f3[k].x - l3[k].x) * ism[k], (f3[k].y - l3[k].y) * ism[k]);
          am[0] += bi.x * bi.x + bi.y * bi.y;
        } else {
          f3[k] = make_double2(0.0, 0.0);
        }
      }
      // (x0 is not carried in registers across the element loop below - 28 VGPRs the loop's two interleaved triangles need,
      //  spilled to scratch in round 3: its own rows are read back from the staged copy, which the loop only reads)
      __syncthreads();
      CT_STAMP(2)
      // (one triangle at a time: beside f3 / ism / the prefetched metadata the two interleaved triangles of the other
      //  applications did not fit - 180 B of scratch per lane in round 3; this application runs once per launch)
      atomic_accumulate<MDQ_CORR_MX0_INTERLEAVE>(v, Yd, tm, [&](int, const Geo& g, const ElemIdx& E, int, double2(&ye)[6]) {
        double2 xe[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) xe[i] = Pl[E.dof[i]];
        elem_mass(g, xe, ye);
      });
      __syncthreads();
      CT_STAMP(3)
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        r[k] = p[k] = x[k] = make_double2(0.0, 0.0);
        if (row < n2) {
          const double2 ax = Yl[row];
          x[k] = Pl[row];
          r[k] = make_double2((f3[k].x - ax.x) * ism[k], (f3[k].y - ax.y) * ism[k]);  // 0 on constrained rows
          p[k] = r[k];
          am[1] += r[k].x * r[k].x + r[k].y * r[k].y;
          if (ism[k] != 0.0) x[k] = make_double2(x[k].x / ism[k], x[k].y / ism[k]);  // scaled unknown S x
        }
      }
      block_sum<2>(am, red);
      bb = am[0];
      if (tid == 0) ccnt[2] = bb;
    }
    CT_STAMP(4)
    {
      const double tol2 = d.rtol * d.rtol * bb;
      double rr = am[1];
      if (rr > tol2 && bb != 0.0) {
        int it = 0;
        while (it < d.maxit_m) {
          ++it;
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const int row = tid + k * WG;
            if (row < n2) {
              Pl[row] = make_double2(p[k].x * ism[k], p[k].y * ism[k]);
              Yl[row] = make_double2(0.0, 0.0);
            }
          }
          __syncthreads();
          CT_STAMP(5)
          atomic_accumulate<true>(v, Yd, tm, [&](int, const Geo& g, const ElemIdx& E, int, double2(&ye)[6]) {
            double2 xe[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) xe[i] = Pl[E.dof[i]];
            elem_mass(g, xe, ye);
          });
          __syncthreads();
          CT_STAMP(6)
          double a1[1] = {0.0};
          double2 q[MF_ROWS];
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            const int row = tid + k * WG;
            q[k] = make_double2(0.0, 0.0);
            if (row < n2) {
              const double2 yv = Yl[row];
              q[k] = make_double2(yv.x * ism[k], yv.y * ism[k]);
              a1[0] += p[k].x * q[k].x + p[k].y * q[k].y;
            }
          }
          block_sum1<1>(a1, red, rsel);
          CT_STAMP(7)
          if (!(a1[0] > 0.0)) break;
          const double alpha = rr / a1[0];
          double a2[1] = {0.0};
#pragma unroll
          for (int k = 0; k < MF_ROWS; ++k) {
            x[k] = make_double2(x[k].x + alpha * p[k].x, x[k].y + alpha * p[k].y);
            r[k] = make_double2(r[k].x - alpha * q[k].x, r[k].y - alpha * q[k].y);
            a2[0] += r[k].x * r[k].x + r[k].y * r[k].y;
          }
          block_sum1<1>(a2, red, rsel);
          CT_STAMP(8)
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
    {
      double2 us[MF_ROWS];
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) us[k] = xs[rc[k]];
      double2* cnew = cring + (int64_t)rp * d.N2;
#pragma unroll
      for (int k = 0; k < MF_ROWS; ++k) {
        const int row = tid + k * WG;
        if (row < n2) {
          const double2 un = (ism[k] != 0.0) ? make_double2(x[k].x * ism[k], x[k].y * ism[k]) : x[k];
          v.u_n[row] = un;
          cnew[row] = (ism[k] != 0.0) ? make_double2(un.x - us[k].x, un.y - us[k].y) : make_double2(0.0, 0.0);
        }
      }
    }
    if (tid == 0) {
      ccnt[0] = (double)(nc < 3 ? nc + 1 : 3);
      ccnt[1] = (double)((rp + 1) % 3);
      ccnt[3] = (double)((cstep + 1) & 1023);
      if (fresh0) {   // the history counters of the other operator modes, as reset_history_kernel leaves them
        double* hcnt = reinterpret_cast<double*>(cring + 5 * (int64_t)d.N2);
        hcnt[0] = hcnt[1] = 0.0;
      }
    }
    for (int i = tid; i < nv; i += WG) v.p_n[i] = pnew[i];
    __syncthreads();
    CT_STAMP(9)
    double dr, li;
    forces(v, v.mu, v.u_n, v.p_n, red, dr, li);
    CT_STAMP(10)
    if (tid == 0) {
      drag[(int64_t)b * nsteps + step] = dr;
      lift[(int64_t)b * nsteps + step] = li;
    }
  }
  if (tid == 0 && iters) iters[3 * b + 2] = (fresh0 ? 0 : iters[3 * b + 2]) + it_m;
}

}  // namespace mdq
