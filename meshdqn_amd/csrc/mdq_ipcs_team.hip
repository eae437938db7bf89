// IPCS: two workgroups per environment - the team barrier and sums, evolve_team_kernel (mode 4), evolve_team_tiles_kernel
// (mode 7), team_reset_kernel and their launchers.  Included by mdq_tu_ipcs_tiles.hip only, behind evolve_kernel.
namespace mdq {

#ifdef MDQ_T5_TRACE
// debug build only: the host half of the T5 stamps (buffer and macro: mdq_ipcs_ops.hip)
extern "C" MDQ_API int mdq_t5_trace_host(long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mdq_t5_trace_buf), sizeof(long long) * 8) != hipSuccess) return -1;
  if (reset) { long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(mdq_t5_trace_buf), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
#endif

// ================================================================== assembled operators, TWO workgroups per environment
//
// evolve_kernel<0> gives one workgroup - one CU - to an environment: with the BASELINE batch of 128 environments half of
// the chip idles, and on meshes whose operators no longer fit a CU's caches (BASELINE configs[4]: ys930 red-refined,
// 6 MB of velocity blocks per environment) the step is bound by what ONE CU pulls from L2 / HBM (~22 GB/s).  Here a TEAM
// of two workgroups shares an environment: element loops, row loops and SELL slices are dealt out alternately
// (global thread id = rank * WG + tid, stride 2 WG), all vectors live in the environment's workspace slab, and every
// barrier that separates a producer phase from a consumer phase is a TEAM barrier: agent-scope release by every wave,
// workgroup barrier, one arrival counter per team polled by one lane (bounded spin), workgroup barrier, agent-scope
// acquire - correct for any placement of the two workgroups (cdna_hip_programming.md, Guideline 16).  Reductions: each
// workgroup's deterministic block sum goes to the team's slot array and both workgroups add the two partials in rank
// order: every thread of the team sees the same bits.  The pressure solve (3 322 unknowns, LDS-resident vectors, direct
// factors or CG) stays with rank 0.  Same arithmetic as evolve_kernel<0> except for the association of the reductions - by
// construction: the step phases and the two Krylov solvers ARE evolve_kernel's code (velocity_rhs, bicgstab_velocity,
// pressure_solve, correction_rhs, cg_mass, update_velocity), instantiated for the team's row group (TeamRows) and the SELL
// products over the team's slices.  The kernel keeps its row ranges, the time-out handling (team_failed) and rank 0's solve.
struct Team {
  int rank;
  unsigned* ctr;     // [0] arrivals of the team, [1] set when a bounded spin ran out (the step's forces become NaN)
  double* slot;      // [2 parities][TEAM][4] partial sums
  unsigned epoch;
  int par;
  bool local;        // both workgroups run on the same XCD (team_place): the barrier need not go beyond that XCD's L2
  int rbeg, rend;    // mode 7: the rows of this workgroup in the vector passes and the epilogues
};
// The agent-scope fences of the general barrier write the XCD's L2 back and invalidate it - what an environment re-reads in
// every operator application (0.7 MB of element metadata on the refined mesh) is gone after every barrier: measured on the
// element tiles, 215 barriers per step, 27.3 ms per step of 128 refined meshes against 11.5 ms for ONE workgroup per
// environment.  Two workgroups on the SAME XCD share its L2, and the vector L1 of a CU is write-through: waiting for the
// own stores (vmcnt) and invalidating the own L1 behind the barrier is all the coherence they need.  The launcher's block
// numbering puts a team on block ids 8 apart - the same XCD under the dispatcher's round-robin - and every team CHECKS it
// (hardware register XCC_ID, exchanged through the general barrier at kernel start): any other placement keeps the
// general protocol.
__device__ __forceinline__ unsigned xcc_id() {
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  return x & 0xFu;
}
__device__ __forceinline__ void team_sync(Team& t) {
  if (t.local)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // every wave: its stores have reached the XCD's L2
  else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");     // every wave: its stores are visible device-wide
  __syncthreads();
  ++t.epoch;
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(t.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned target = t.epoch * TEAM;
    if (!__hip_atomic_load(t.ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
      unsigned spins = 0;
      while (__hip_atomic_load(t.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(4);
        if (++spins > (1u << 22)) {                        // the partner never arrived (not resident?): give up, loudly
          __hip_atomic_store(t.ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
    }
  }
  __syncthreads();
  if (t.local)
    // every wave: no stale lines of the partner's data in this CU's L1.  Device scope (sc1): the partner is ANOTHER workgroup on
    // another CU, and the workgroup-scope form (sc0) left this CU's lines in place - a mesh small enough for its vectors and the
    // reduction slots to stay in the L1 between two barriers (under ~500 rows: tests/test_ipcs_ladder_gpu.py, mode 7) then read
    // the values of the application before; larger meshes only evicted them in time.  Memory local to the device is never
    // stale in the XCD's L2, so nothing there is dropped: the L2 keeps what an environment re-reads.
    asm volatile("buffer_inv sc1" ::: "memory");
  else
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
// the placement check at kernel start (through the general barrier); `ids`: two words of the environment's slab
__device__ __forceinline__ void team_place(Team& t, unsigned* ids, int general) {
  t.local = false;
  if (threadIdx.x == 0) __hip_atomic_store(ids + t.rank, xcc_id() + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  team_sync(t);
  const unsigned i0 = __hip_atomic_load(ids, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned i1 = __hip_atomic_load(ids + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  static_assert(TEAM == 2, "two ids");
  t.local = i0 == i1 && !(general & 1);     // (`general` bit 0: MDQ_TEAM_GENERAL_BARRIER=1 keeps the placement-independent protocol - tests)
}
template <int N>
__device__ __forceinline__ void team_sum(double (&v)[N], double* red, Team& t) {
  static_assert(N <= 4, "slot capacity");
  block_sum<N>(v, red);
  double* mine = t.slot + (t.par * TEAM + t.rank) * 4;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) mine[n] = v[n];
  }
  team_sync(t);
  const double* s0 = t.slot + (t.par * TEAM) * 4;
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = s0[n] + s0[4 + n];
  t.par ^= 1;
}
// the row group of a team (see "Krylov solvers"): this thread's rows are first, first + stride, .. below `end` - dealt out
// over the 2 WG threads of the team (mode 4) or the workgroup's contiguous half (mode 7) -, barriers and sums are the team's
struct TeamRows {
  Team& T;
  int first, end, stride;
  template <class F>
  __device__ __forceinline__ void rows(int n, F f) const {
    for (int i = first; i < min(end, n); i += stride) f(i);
  }
  __device__ __forceinline__ void sync() const { team_sync(T); }
  template <int N>
  __device__ __forceinline__ void sum(double (&acc)[N], double* red) const { team_sum<N>(acc, red, T); }
};

// A bounded spin of this team ran out in this launch (the partner workgroup was not resident for ~2^22 polls: another process
// or another stream held its CU).  Read by every thread behind a team barrier.  The step that sees it does NOT advance u_n / p_n,
// drops the initial-guess history (the vectors computed past the broken barrier are finite garbage), reports NaN forces for
// this and every later step of the launch, and the host raises (ipcs_batch.py / vec_env.py: `MeshDQNHipError`).
__device__ __forceinline__ bool team_failed(const Team& t) {
  return __hip_atomic_load(t.ctr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}
// bit 1 of the kernels' `general` argument (MDQ_TEAM_TEST_ABSENT_PARTNER=1, tests only): the second workgroup of
// environment 0 leaves at once - the time-out path of the barrier, forced
__device__ __forceinline__ bool team_test_absent(int general, int b, int rank) { return (general & 2) && b == 0 && rank == 1; }

static __global__ void team_reset_kernel(mdq_ipcs_desc d) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  double* w = d.work + (int64_t)b * work_per_env(d.NV, d.NT, d.NE);
  double* spare = w + 12 * (int64_t)d.NT + 12 * (int64_t)d.N2 + d.NV;
  unsigned* ctr = reinterpret_cast<unsigned*>(spare + 8);
  ctr[0] = ctr[1] = 0u;
}

template <bool K1_LDS>
__global__ __launch_bounds__(WG) void evolve_team_kernel(mdq_ipcs_desc d, int nsteps, double* drag, double* lift,
                                                          int32_t* iters, int general, const double* inflow_scale) {
  extern __shared__ __align__(16) double smem[];
  // teams on neighbouring-by-8 block ids: with the dispatcher's round-robin both workgroups tend to share an XCD's L2
  // (a speed choice only: the protocol is placement-independent)
  const int q = blockIdx.x / (8 * TEAM), r8 = blockIdx.x % (8 * TEAM);
  const int b = q * 8 + (r8 & 7), rank = r8 >> 3;
  if (b >= d.B || team_test_absent(general, b, rank)) return;
  const int tid = threadIdx.x, gt = rank * WG + tid;
  constexpr int GS = TEAM * WG;
  const EnvView v = env_view(d, b);
  const int n2 = v.n2, nv = v.nv;
  const LdsPlan P = lds_plan(d.N2, d.NV, d.NSE1);
  double* red = smem;
  double* U = smem + 64;
  const PrsLds L = prs_lds(U, P, d);
  double* w = v.work;
  double2* escr2 = reinterpret_cast<double2*>(w);
  double* escr1 = w;
  double2* xs = reinterpret_cast<double2*>(w + 12 * (int64_t)d.NT);
  double2* vr = xs + d.N2;
  double2* vh = vr + d.N2;
  double2* vp = vh + d.N2;
  double2* vv = vp + d.N2;
  double2* vt = vv + d.N2;
  const VelHist H = vel_hist(d, w);
  double* hcnt = H.cnt;
  double* pnew = reinterpret_cast<double*>(vt + d.N2);
  double* spare = pnew + d.NV;
  Team T;
  T.rank = rank;
  T.ctr = reinterpret_cast<unsigned*>(spare + 8);
  T.slot = spare + 9;
  T.epoch = 0;
  T.par = 0;
  const KrylovLds ka{2 * sizeof(double) * (size_t)P.NVp, L.lK, sizeof(double) * (size_t)P.NVp, nullptr, 0, 0};
  const double a = v.rho / v.dt;
  int it_u = 0, it_p = 0, it_m = 0;
  const TeamRows rg{T, gt, n2, GS};
  const VelCtx vc{xs, vr, vh, vp, vv, vt};
  const MassCtx mc{xs, vr, vp, vv, vp};
  const int lane = tid & 63, gw = rank * NWAVE + (tid >> 6);
  constexpr int GW = TEAM * NWAVE;
  // SELL operator applications over the team's slices
  auto spmv_vel = [&](const double2* x, auto epi) {
    const int nsl = (n2 + 63) >> 6;
    const double4* A4 = reinterpret_cast<const double4*>(v.A1);
    for (int s = gw; s < nsl; s += GW) {
      const int base = v.sl2_off[s], wd = (v.sl2_off[s + 1] - base) >> 6;
      const double4* aa = A4 + base + lane;
      const int32_t* c = v.sl2_col + base + lane;
      double y0 = 0.0, y1 = 0.0;
#pragma unroll 4
      for (int j = 0; j < wd; ++j) {
        const double4 av = aa[j * 64];
        const double2 xv = x[c[j * 64]];
        y0 += av.x * xv.x + av.y * xv.y;
        y1 += av.z * xv.x + av.w * xv.y;
      }
      const int row = (s << 6) + lane;
      if (row < n2) epi(row, y0, y1);
    }
  };
  auto spmv_mass = [&](const double2* x, auto epi) {
    const int nsl = (n2 + 63) >> 6;
    for (int s = gw; s < nsl; s += GW) {
      const int base = v.sl2_off[s], wd = (v.sl2_off[s + 1] - base) >> 6;
      const double* aa = v.Ms + base + lane;
      const int32_t* c = v.sl2_col + base + lane;
      double y0 = 0.0, y1 = 0.0;
#pragma unroll 4
      for (int j = 0; j < wd; ++j) {
        const double av = aa[j * 64];
        const double2 xv = x[c[j * 64]];
        y0 += av * xv.x;
        y1 += av * xv.y;
      }
      const int row = (s << 6) + lane;
      if (row < n2) epi(row, y0, y1);
    }
  };
  team_place(T, reinterpret_cast<unsigned*>(spare + 25), general);
  for (int step = 0; step < nsteps; ++step) {
    const double ai = inflow_factor(inflow_scale, b, nsteps, step);
    // ---------------- step 1: tentative velocity
    rhs1_elements(v, d, v.u_n, v.p_n, escr2, a, v.mu, gt, GS);
    team_sync(T);
    double acc[2] = {0.0, 0.0};
    const int nhist = (int)hcnt[0];
    velocity_rhs<false>(rg, spmv_vel, v, vc, ai, escr2, nhist, H, red, acc);
    it_u += bicgstab_velocity(rg, spmv_vel, v, vc, d.rtol, d.maxit_u, acc[0], acc[1], red);
    team_sync(T);
    rg.rows(n2, [&](int i) { history_shift(nhist, H, xs, i); });
    // ---------------- step 2: pressure (element loop by the team, the solve by rank 0)
    rhs2_elements(v, d, xs, v.p_n, escr1, gt, GS);
    team_sync(T);
    if (rank == 0) {
      if (tid == 0) hcnt[0] = (double)(nhist < 5 ? nhist + 1 : 5);
      it_p += pressure_solve<K1_LDS, true>(v, d, b, escr1, L, pnew, ka, red, [](int) {});
    }
    team_sync(T);
    // ---------------- step 3: velocity correction
    rhs3_elements(v, d, xs, pnew, v.p_n, escr2, gt, GS);
    team_sync(T);
    double am[2] = {0.0, 0.0};
    correction_rhs<false>(rg, spmv_mass, v, mc, ai, escr2, red, am);
    it_m += cg_mass<false>(rg, spmv_mass, v, mc, d.rtol, d.maxit_m, am[0], am[1], red);
    team_sync(T);
    // ---------------- update state + probes
    if (team_failed(T)) {       // (see team_failed: the state stays the last good one, NaN forces from here on)
      if (rank == 0 && tid == 0) {
        hcnt[0] = 0.0;
        if (d.status) atomicOr(d.status + b, MDQ_IPCS_TEAM_TIMEOUT);
        for (int s_ = step; s_ < nsteps; ++s_) drag[(int64_t)b * nsteps + s_] = lift[(int64_t)b * nsteps + s_] = __builtin_nan("");
      }
      break;
    }
    update_velocity(rg, v, xs);
    for (int i = gt; i < nv; i += GS) v.p_n[i] = pnew[i];
    team_sync(T);
    if (rank == 0) {
      double dr, li;
      forces(v, v.mu, v.u_n, v.p_n, red, dr, li);
      if (tid == 0) {
        const bool failed = team_failed(T);
        drag[(int64_t)b * nsteps + step] = failed ? __builtin_nan("") : dr;
        lift[(int64_t)b * nsteps + step] = failed ? __builtin_nan("") : li;
      }
    }
  }
  if (rank == 0 && tid == 0 && iters) {
    iters[3 * b + 0] += it_u;
    iters[3 * b + 1] += it_p;
    iters[3 * b + 2] += it_m;
  }
}

// MDQ_TEAM_GENERAL_BARRIER=1 (read per launch): the teams keep the placement-independent agent-scope barrier even when both
// workgroups share an XCD - the same arithmetic, so the same bits (tests/test_ipcs_gpu.py), at 2-3x the step time
static int team_general_barrier() {
  return (std::getenv("MDQ_TEAM_GENERAL_BARRIER") != nullptr ? 1 : 0) | (std::getenv("MDQ_TEAM_TEST_ABSENT_PARTNER") != nullptr ? 2 : 0);
}

template <bool K1_LDS>
static hipError_t launch_evolve_team(const mdq_ipcs_desc* d, size_t lds, int nsteps, double* drag, double* lift,
                                     int32_t* iters, const double* inflow_scale, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&evolve_team_kernel<K1_LDS>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(team_reset_kernel, dim3((d->B + 63) / 64), dim3(64), 0, stream, *d);
  const int teams8 = (d->B + 7) / 8;                       // blocks: groups of 8 environments x TEAM ranks
  hipLaunchKernelGGL((evolve_team_kernel<K1_LDS>), dim3(teams8 * 8 * TEAM), dim3(WG), lds, stream, *d, nsteps, drag, lift,
                     iters, team_general_barrier(), inflow_scale);
  return hipGetLastError();
}

// ================================================================== element tiles, TWO workgroups per environment (mode 7)
//
// Mode 5 gives an environment ONE workgroup, and what bounds it on the refined mesh is that workgroup's memory-level
// parallelism (22 GB/s per CU, HISTORY 8.5), not the chip: at the BASELINE batch of 128 environments half of the CUs idle,
// and 256 environments take 14.2 ms where 128 take 11.3.  Here the two workgroups of a team (the protocol of mode 4: team
// barriers, reductions through the team's slots) share an environment's tile operators: the chunks of a tile application
// are dealt out alternately, every workgroup accumulates its chunks' row sums into ITS OWN vector of the slab (in fixed
// order, as mode 5 does), and behind one team barrier the rows - dealt out over the 1 024 threads of the team like every
// vector pass - add the two partial sums in rank order and run the caller's epilogue.  Bitwise reproducible run to run;
// NOT bitwise mode 5: a row's sum is (chunks 0, 2, 4, ..) + (chunks 1, 3, 5, ..) instead of chunk after chunk.  Without
// tile maps (index data built on the device) the element results go to the slab's element scratch, triangles and rows
// dealt out over the team.  Right-hand sides, the pressure solve (rank 0) and the probes: as in mode 4, and the step phases
// and solvers are the same code as evolve_kernel<5>'s (tile forms of velocity_rhs / correction_rhs, the staged cg_mass),
// instantiated for the team's row group over each workgroup's contiguous half of the rows and tile_apply_team.
// Which rows a workgroup's chunks touch (t0 / t1: one byte per row) and which entries of its chunks' row lists are the first
// touch of their row in the workgroup's walk (first: one byte per entry) - built once per launch from the row lists: a
// tile application then neither zero-fills the two accumulation vectors nor reads a partial sum that does not exist
// (per application of the refined mesh 1.32 -> 0.57 MB of the ~2.9 MB the workgroups move; the zero fill + full reads were
// what the first version of mode 7 moved more than mode 5, 38.4 against 32.1 GB per step of 128 environments).
struct TeamTouch {
  unsigned char *t0, *t1, *first;   // (first == nullptr: no row lists - zero fill and full reads)
  int stride;                       // entries of `first` per chunk
};
__device__ inline void team_touch_setup(const EnvView& v, const Team& T, TeamTouch& tt) {
  if (!v.mf_rlist || !v.tiles) {
    tt.first = nullptr;
    return;
  }
  const int tid = threadIdx.x, n = v.n2, nch = (v.nt + MF_CH - 1) / MF_CH;
  unsigned char* tm = T.rank ? tt.t1 : tt.t0;
  for (int row = tid; row < n; row += WG) tm[row] = 0;
  __syncthreads();
  for (int chunk = T.rank; chunk < nch; chunk += TEAM) {
    const int2* rl = reinterpret_cast<const int2*>(v.mf_rlist) + (size_t)chunk * v.NRL;
    const int nr = v.mf_rcnt[chunk];
    unsigned char* fbc = tt.first + (size_t)chunk * tt.stride;
    for (int k = tid; k < nr; k += WG) {      // (a row appears once per chunk: its byte is read and set by one thread)
      const int row = rl[k].x & 0x3FFFFFFF;
      fbc[k] = tm[row] == 0;
      tm[row] = 1;
    }
    __syncthreads();
  }
}

template <class ElemOp, class Epi>
__device__ __forceinline__ void tile_apply_team(const EnvView& v, Team& T, bool packed, double2* es, double2* y0v, double2* y1v,
                                                const TeamTouch& tt, const double2* gx, ElemOp op, Epi epi) {
  const int tid = threadIdx.x, n = v.n2, gt = T.rank * WG + tid;
  constexpr int GS = TEAM * WG;
  if (!v.tiles) {
    double2* es2 = reinterpret_cast<double2*>(v.work);
    for (int e = gt; e < v.nt; e += GS) {
      double2 xe[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) xe[i] = gx[v.cell_dofs[i * v.NT + e]];
      const Geo g = load_geo(v, e);
      double2 ye[6];
      op(e, g, (int)v.cell_outflow[e], xe, ye);
#pragma unroll
      for (int i = 0; i < 6; ++i) es2[e * 6 + i] = ye[i];
    }
    team_sync(T);
    for (int row = T.rbeg + tid; row < T.rend; row += WG) {
      double2 a = make_double2(0.0, 0.0);
      for (int s = v.g2_ptr[row]; s < v.g2_ptr[row + 1]; ++s) {
        const double2 c = es2[v.g2_src[s]];
        a.x += c.x;
        a.y += c.y;
      }
      epi(row, a.x, a.y);
    }
    return;       // (the caller's team reduction is the barrier in front of the next use of the element scratch)
  }
  tile_chunks_global(v, packed, es, T.rank ? y1v : y0v, gx, op, T.rank, TEAM, false, tt.first, tt.stride);
  team_sync(T);
  constexpr int EB = 4;
  const bool masks = tt.first != nullptr && v.mf_rlist;
  for (int row0 = T.rbeg + tid; row0 < T.rend; row0 += EB * WG) {
    double2 a[EB], c[EB];
    unsigned m0 = 0xFu, m1 = 0xFu;
    if (masks) {
      // a partial sum exists only where the workgroup's chunks touch the row (mostly ONE of the two: a row meets 1.2 chunks
      // on average) - the other vector's entry is stale and not read
      m0 = m1 = 0u;
#pragma unroll
      for (int k = 0; k < EB; ++k) {
        const int rc = min(row0 + k * WG, n - 1);
        m0 |= tt.t0[rc] ? 1u << k : 0u;
        m1 |= tt.t1[rc] ? 1u << k : 0u;
      }
    }
#pragma unroll
    for (int k = 0; k < EB; ++k) {
      a[k] = c[k] = make_double2(0.0, 0.0);
      if ((m0 >> k) & 1u) a[k] = y0v[min(row0 + k * WG, n - 1)];
      if ((m1 >> k) & 1u) c[k] = y1v[min(row0 + k * WG, n - 1)];
    }
#pragma unroll
    for (int k = 0; k < EB; ++k)
      if (row0 + k * WG < T.rend) epi(row0 + k * WG, a[k].x + c[k].x, a[k].y + c[k].y);
  }
}

template <bool K1_LDS>
__global__ __launch_bounds__(WG) void evolve_team_tiles_kernel(mdq_ipcs_desc d, int nsteps, double* drag, double* lift,
                                                                int32_t* iters, int general, const double* inflow_scale) {
  extern __shared__ __align__(16) double smem[];
  const int q = blockIdx.x / (8 * TEAM), r8 = blockIdx.x % (8 * TEAM);
  const int b = q * 8 + (r8 & 7), rank = r8 >> 3;
  if (b >= d.B || team_test_absent(general, b, rank)) return;
  const int tid = threadIdx.x, gt = rank * WG + tid;
  constexpr int GS = TEAM * WG;
  const EnvView v = env_view(d, b);
  const int n2 = v.n2, nv = v.nv;
  const LdsPlan P = lds_plan(d.N2, d.NV, d.NSE1);
  double* red = smem;
  double* U = smem + 64;
  // pressure view of the union (rank 0 only) | velocity view: the element tile (+ the staged rows of a chunk)
  const PrsLds L = prs_lds(U, P, d);
  double2* es = reinterpret_cast<double2*>(U);
  double* w = v.work;
  double2* escr2 = reinterpret_cast<double2*>(w);
  double* escr1 = w;
  double2* xs = reinterpret_cast<double2*>(w + 12 * (int64_t)d.NT);
  double2* vr = xs + d.N2;
  double2* vh = vr + d.N2;
  double2* vp = vh + d.N2;
  double2* vv = vp + d.N2;
  double2* vt = vv + d.N2;
  const VelHist H = vel_hist(d, w);
  double* hcnt = H.cnt;
  double2* y0v = reinterpret_cast<double2*>(w + work_ytmp_offset(d.NV, d.NT, d.NE));   // the workgroups' accumulation vectors
  double2* y1v = y0v + d.N2 + 1;
  TeamTouch tt;
  tt.t0 = reinterpret_cast<unsigned char*>(w + work_touch_offset(d.NV, d.NT, d.NE));
  tt.t1 = tt.t0 + d.N2;
  tt.first = tt.t1 + d.N2;
  tt.stride = (int)work_touch_row_cap(d.NV, d.NE);
  double2* stage = vh;                                   // the mass solve's S^-1 p (vh is free there)
  double* pnew = reinterpret_cast<double*>(vt + d.N2);
  double* spare = pnew + d.NV;
  Team T;
  T.rank = rank;
  T.ctr = reinterpret_cast<unsigned*>(spare + 8);
  T.slot = spare + 9;
  T.epoch = 0;
  T.par = 0;
  {
    // the rows of the vector passes and the epilogues: CONTIGUOUS halves (8.45 -> 8.2 ms per step of 128 refined meshes
    // against rows dealt out alternately over the 1 024 threads: the two CUs no longer write into the same lines).  With
    // an odd number of chunks workgroup 0 applies one more, but moving rows to the other workgroup to make up for it was
    // measured slower both ways (0.32 / 0.61 of the rows to workgroup 0: 9.1 / 8.8 ms)
    int split = n2 / 2;
    split &= ~63;
    T.rbeg = rank ? split : 0;
    T.rend = rank ? n2 : split;
  }
  const KrylovLds ka{2 * sizeof(double) * (size_t)P.NVp, L.lK, sizeof(double) * (size_t)P.NVp, U,
                     max(P.prs_vec_bytes + (K1_LDS ? P.prs_mat_bytes : 0), tile_lds_bytes(d)), P.NVp};
  const double a = v.rho / v.dt, mu = v.mu;
  const bool packed = d.N2 <= 4096;
  int it_u = 0, it_p = 0, it_m = 0;
  const TeamRows rg{T, T.rbeg + tid, T.rend, WG};
  const VelCtx vc{xs, vr, vh, vp, vv, vt};
  const MassCtx mc{xs, vr, vp, vv, stage};
  // y = D^-1 A x (0 on constrained rows) / y = S^-1 M x' on the team's rows
  auto apply_vel = [&](const double2* gx, auto epi) {
    tile_apply_team(
        v, T, packed, es, y0v, y1v, tt, gx,
        [&](int e, const Geo& g, int ko, const double2(&xe)[6], double2(&ye)[6]) { velocity_op(v, a, mu, e, ko, g, xe, ye); },
        [&](int row, double y0, double y1) {
          const bool fl = v.bcu_flag[row] != 0;
          const double2 id = v.idiag1[row];
          epi(row, fl ? 0.0 : y0 * id.x, fl ? 0.0 : y1 * id.y);
        });
  };
  auto apply_mass = [&](const double2* gx, auto epi) {
    tile_apply_team(
        v, T, packed, es, y0v, y1v, tt, gx,
        [&](int, const Geo& g, int, const double2(&xe)[6], double2(&ye)[6]) { elem_mass(g, xe, ye); },
        [&](int row, double y0, double y1) {
          const double is = v.bcu_flag[row] ? 0.0 : 1.0 / v.sdiagM[row];
          epi(row, y0 * is, y1 * is);
        });
  };
  team_place(T, reinterpret_cast<unsigned*>(spare + 25), general);
  if (d.NRL > tt.stride) tt.first = nullptr;       // (cannot happen: a list holds at most min(N2, 6 MF_CH) rows)
  else team_touch_setup(v, T, tt);                  // (published by the team barriers of step 1's right-hand side)
  for (int step = 0; step < nsteps; ++step) {
    const double ai = inflow_factor(inflow_scale, b, nsteps, step);
    // ---------------- step 1: tentative velocity
    rhs1_elements(v, d, v.u_n, v.p_n, escr2, a, mu, gt, GS);
    team_sync(T);
    double acc[2] = {0.0, 0.0};
    const int nhist = (int)hcnt[0];
    velocity_rhs<true>(rg, apply_vel, v, vc, ai, escr2, nhist, H, red, acc);
    it_u += bicgstab_velocity(rg, apply_vel, v, vc, d.rtol, d.maxit_u, acc[0], acc[1], red);
    team_sync(T);
    rg.rows(n2, [&](int i) { history_shift(nhist, H, xs, i); });
    // ---------------- step 2: pressure (element loop by the team, the solve by rank 0)
    rhs2_elements(v, d, xs, v.p_n, escr1, gt, GS);
    team_sync(T);
    if (rank == 0) {
      if (tid == 0) hcnt[0] = (double)(nhist < 5 ? nhist + 1 : 5);
      it_p += pressure_solve<K1_LDS, true>(v, d, b, escr1, L, pnew, ka, red, [](int) {});
    }
    team_sync(T);
    // ---------------- step 3: velocity correction
    rhs3_elements(v, d, xs, pnew, v.p_n, escr2, gt, GS);
    team_sync(T);
    double am[2] = {0.0, 0.0};
    correction_rhs<true>(rg, apply_mass, v, mc, ai, escr2, red, am);
    it_m += cg_mass<true>(rg, apply_mass, v, mc, d.rtol, d.maxit_m, am[0], am[1], red);
    team_sync(T);
    // ---------------- update state + probes
    if (team_failed(T)) {       // (see team_failed: the state stays the last good one, NaN forces from here on)
      if (rank == 0 && tid == 0) {
        hcnt[0] = 0.0;
        if (d.status) atomicOr(d.status + b, MDQ_IPCS_TEAM_TIMEOUT);
        for (int s_ = step; s_ < nsteps; ++s_) drag[(int64_t)b * nsteps + s_] = lift[(int64_t)b * nsteps + s_] = __builtin_nan("");
      }
      break;
    }
    update_velocity(rg, v, xs);
    for (int i = gt; i < nv; i += GS) v.p_n[i] = pnew[i];
    team_sync(T);
    if (rank == 0) {
      double dr, li;
      forces(v, v.mu, v.u_n, v.p_n, red, dr, li);
      if (tid == 0) {
        const bool failed = team_failed(T);
        drag[(int64_t)b * nsteps + step] = failed ? __builtin_nan("") : dr;
        lift[(int64_t)b * nsteps + step] = failed ? __builtin_nan("") : li;
      }
    }
  }
  if (rank == 0 && tid == 0 && iters) {
    iters[3 * b + 0] += it_u;
    iters[3 * b + 1] += it_p;
    iters[3 * b + 2] += it_m;
  }
}

template <bool K1_LDS>
static hipError_t launch_evolve_team_tiles(const mdq_ipcs_desc* d, size_t lds, int nsteps, double* drag, double* lift,
                                           int32_t* iters, const double* inflow_scale, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&evolve_team_tiles_kernel<K1_LDS>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(team_reset_kernel, dim3((d->B + 63) / 64), dim3(64), 0, stream, *d);
  const int teams8 = (d->B + 7) / 8;                       // blocks: groups of 8 environments x TEAM ranks
  hipLaunchKernelGGL((evolve_team_tiles_kernel<K1_LDS>), dim3(teams8 * 8 * TEAM), dim3(WG), lds, stream, *d, nsteps, drag,
                     lift, iters, team_general_barrier(), inflow_scale);
  return hipGetLastError();
}

}  // namespace mdq
