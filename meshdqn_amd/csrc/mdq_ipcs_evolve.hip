// IPCS: evolve_kernel (one workgroup per environment, all steps in one launch: modes 0 / 1 / 5) and launch_evolve.
// Included by mdq_tu_ipcs_assembled.hip and mdq_tu_ipcs_tiles.hip, behind the phases of a time step.
namespace mdq {

// PG: the four pressure CG vectors live in the workspace slab as well (they alias the velocity Krylov vectors, idle during
// step 2) - a mesh whose pressure vectors exceed the LDS (NV > ~4000) still steps; modes 0 / 5 only, K1_LDS = false.
template <int MODE, bool K1_LDS, bool PG = false>
__global__ __launch_bounds__(WG) void evolve_kernel(mdq_ipcs_desc d, int nsteps, double* drag, double* lift,
                                                     int32_t* iters, const double* inflow_scale) {
  static_assert(!PG || (!K1_LDS && (MODE == 0 || MODE == 5)), "global pressure vectors: modes 0 / 5 without the LDS matrix");
  extern __shared__ __align__(16) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const EnvView v = env_view(d, b);
  const int n2 = v.n2, nv = v.nv;
  const LdsPlan P = lds_plan(d.N2, d.NV, d.NSE1);

  double* red = smem;  // 64 doubles
  double* U = smem + 64;

  // workspace carve-up (global; stays in this CU's L2 slice)
  double* w = v.work;
  double2* escr2 = reinterpret_cast<double2*>(w);  // 6*NT double2 (aliased as 3*NT doubles for step 2)
  double* escr1 = w;
  double2* xs = reinterpret_cast<double2*>(w + 12 * (int64_t)d.NT);
  double2* vr = xs + d.N2;
  double2* vh = vr + d.N2;
  double2* vp = vh + d.N2;
  double2* vv = vp + d.N2;
  double2* vt = vv + d.N2;
  // pressure view of the union (PG: the vectors are the idle velocity vectors; 2 N2 doubles each >= NV)
  PrsLds L = prs_lds(U, P, d);
  if (PG) {
    L.x = reinterpret_cast<double*>(vr);
    L.r = reinterpret_cast<double*>(vh);
    L.p = reinterpret_cast<double*>(vp);
    L.q = reinterpret_cast<double*>(vv);
  }
  const VelHist H = vel_hist(d, w);  // u* history of the velocity solve
  double* hcnt = H.cnt;
  double* pnew = reinterpret_cast<double*>(vt + d.N2);
  // velocity view of the union
  double2* L0 = reinterpret_cast<double2*>(U);
  double2* L1 = L0 + P.N2p;

  VelCtx vc;
  vc.x = xs;
  vc.rh = vh;
  vc.vv = vv;
  vc.t = vt;
  vc.a = v.rho / v.dt;
  vc.mu = v.mu;
  constexpr bool MF = MODE == 5;   // the element-tile operators
  double2* ytmp = reinterpret_cast<double2*>(w + work_ytmp_offset(d.NV, d.NT, d.NE));   // mode 5: accumulation vector
  vc.es = MODE == 5 ? L0 : L1;
  vc.yt = ytmp;
  vc.packed = d.N2 <= 4096;
  vc.p = MODE == 1 ? L0 : vp;    // (modes 0 / 5: the gathers read the Krylov vectors themselves, in global memory)
  vc.r = MODE == 1 ? L1 : vr;
  MassCtx mc;
  mc.x = xs;
  mc.r = vr;
  mc.q = vv;
  mc.es = MODE == 5 ? L0 : L1;
  mc.yt = ytmp;
  mc.packed = d.N2 <= 4096;
  mc.p = MODE == 1 ? L0 : vp;
  mc.gp = MF ? vh : mc.p;   // (mode 5 stages S^-1 p for the gathers: vh is free in the mass solve)

  // (PG: vectors in the slab - L.p is a 2 N2-double vector there -, the preconditioner's tables in the LDS they leave free;
  //  the matrix on the chip: the tile modes only)
  const KrylovLds ka =
      PG ? KrylovLds{2 * sizeof(double) * (size_t)d.N2, U,
                     MODE == 5 ? sizeof(double2) * 6 * MF_CH : tl_extra_bytes(d.NV) + sizeof(double) * NAG * NAG, nullptr, 0, 0}
         : KrylovLds{2 * sizeof(double) * (size_t)P.NVp, L.lK, sizeof(double) * (size_t)P.NVp, MODE == 5 ? U : nullptr,
                     max(P.prs_vec_bytes + (K1_LDS ? P.prs_mat_bytes : 0), MODE == 5 ? tile_lds_bytes(d) : (size_t)0), P.NVp};

  const WgRows rg;
  auto op_vel = [&](const double2* gx, auto epi) { apply_velocity<MODE>(v, vc, gx, epi); };
  auto op_mass = [&](const double2* gx, auto epi) { apply_mass<MODE>(v, mc, gx, epi); };

  int it_u = 0, it_p = 0, it_m = 0;
  const double* frow = PG ? inflow_row_lane(inflow_scale, b, nsteps) : nullptr;
#ifdef MDQ_PROFILE
  long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tprev = __builtin_amdgcn_s_memtime();
#endif
  auto stamp = [&](int k) { MDQ_STAMP(k) };
  __syncthreads();

  for (int step = 0; step < nsteps; ++step) {
    // ---------------- step 1: tentative velocity  (flow_solver.py:106-112, solve 1 of :378-380)
    MDQ_STAMP(7)
    rhs1_elements(v, d, v.u_n, v.p_n, escr2, v.rho / v.dt, v.mu);
    __syncthreads();
    MDQ_STAMP(0)
    double acc[2] = {0.0, 0.0};
    const int nhist = (int)hcnt[0];
    // (the step's inflow factor is loaded where it is used, here and in front of the correction's rows, rather than held
    //  across the two solves between them)
    double ai = PG ? (frow ? frow[step] : 1.0) : inflow_factor(inflow_scale, b, nsteps, step);
    velocity_rhs<MF>(rg, op_vel, v, vc, ai, escr2, nhist, H, red, acc);   // (mode 5 gathers x0 from xs)
    MDQ_STAMP(1)
    it_u += bicgstab_velocity(rg, op_vel, v, vc, d.rtol, d.maxit_u, acc[0], acc[1], red);
    __syncthreads();
    rg.rows(n2, [&](int i) { history_shift(nhist, H, xs, i); });
    if (tid == 0) hcnt[0] = (double)(nhist < 5 ? nhist + 1 : 5);
    MDQ_STAMP(2)

    // ---------------- step 2: pressure  (flow_solver.py:115-116)
    rhs2_elements(v, d, xs, v.p_n, escr1);
    __syncthreads();
    it_p += pressure_solve<K1_LDS, !PG>(v, d, b, escr1, L, pnew, ka, red, stamp);
    __syncthreads();

    // ---------------- step 3: velocity correction  (flow_solver.py:119-120)
    rhs3_elements(v, d, xs, pnew, v.p_n, escr2);
    __syncthreads();
    double am[2] = {0.0, 0.0};
    ai = PG ? (frow ? frow[step] : 1.0) : inflow_factor(inflow_scale, b, nsteps, step);
    correction_rhs<MF>(rg, op_mass, v, mc, ai, escr2, red, am);
    MDQ_STAMP(5)
    it_m += cg_mass<MF>(rg, op_mass, v, mc, d.rtol, d.maxit_m, am[0], am[1], red);   // (the update below reads own rows: no barrier)
    MDQ_STAMP(6)

    // ---------------- update state + probes  (flow_solver.py:382-389)
    update_velocity(rg, v, xs);
    for (int i = tid; i < nv; i += WG) v.p_n[i] = pnew[i];
    __syncthreads();
    double dr, li;
    forces(v, v.mu, v.u_n, v.p_n, red, dr, li);
    if (tid == 0) {
      drag[(int64_t)b * nsteps + step] = dr;
      lift[(int64_t)b * nsteps + step] = li;
    }
  }
#ifdef MDQ_PROFILE
  if (tid == 0) {
    double* pw = pnew + d.NV;
    for (int k = 0; k < 8; ++k) pw[k] += (double)prof[k];
  }
#endif
  if (tid == 0 && iters) {
    iters[3 * b + 0] += it_u;
    iters[3 * b + 1] += it_p;
    iters[3 * b + 2] += it_m;
  }
}

template <int MODE, bool K1_LDS, bool PG = false>
static hipError_t launch_evolve(const mdq_ipcs_desc* d, size_t lds, int nsteps, double* drag, double* lift,
                                int32_t* iters, const double* inflow_scale, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&evolve_kernel<MODE, K1_LDS, PG>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((evolve_kernel<MODE, K1_LDS, PG>), dim3(d->B), dim3(WG), lds, stream, *d, nsteps, drag, lift,
                     iters, inflow_scale);
  return hipGetLastError();
}

}  // namespace mdq
