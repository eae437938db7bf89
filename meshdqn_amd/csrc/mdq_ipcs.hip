// IPCS Navier-Stokes hot path for gfx950: assembly, time stepping, probes.
//
// One 512-thread workgroup (8 wave64) owns one environment for the whole
// launch: its operators, vectors and element scratch stay in that CU's L2 slice /
// LDS, every synchronisation is a workgroup barrier, every reduction a fixed
// tree (bitwise reproducible), and `nsteps` time steps run inside ONE launch.
//
// Reference semantics restated here (BaratiLab/MeshDQN):
//   flow_solver.py:98-120   UFL forms F1 / a2,L2 / a3,L3
//   flow_solver.py:123-144  Dirichlet BCs + SystemAssembler (symmetric elimination)
//   flow_solver.py:362-396  evolve()
//   probes.py:23-50         drag / lift surface integrals
#include <hip/hip_runtime.h>
#include <cstdlib>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/meshdqn_hip.h"
#include "mdq_internal.h"
#include "mdq_device.h"
#include "mdq_elem.h"

// This file is compiled as several translation units (meshdqn_amd/build.py: -DMDQ_IPCS_PART=k), each instantiating the
// kernels of some operator modes together with their launchers - as ONE unit it took a minute of every rebuild:
//   part 0  the probe kernel here, everything else in fragments that only this part includes: assembly and the matrix-free
//           set-up (mdq_ipcs_setup.hip), the register-resident pressure solvers of mode 3 (mdq_ipcs_pcg_reg.hip), the three
//           kernels of mode 3 (mdq_ipcs_mode3.hip), the inflow profile and the inlet map (mdq_ipcs_inflow.hip), the error
//           state and the entry points with the launch sequence of mode 3 (mdq_ipcs_entry.hip)
//   part 1  evolve_kernel<0 / 1> (assembled SELL operators)
//   part 2  evolve_kernel<5> (element tiles, global vectors), evolve_team_kernel (mode 4)
//   part 3  the kernels of mode 2 (element tiles, LDS / register vectors: the reproducible mode of the long runs)
// Without the macro everything is one unit.  Kernels and device tables have internal linkage: every unit that uses the
// reference-element tables owns a copy of them (ensure_tables).
#ifndef MDQ_IPCS_PART
#define MDQ_IPCS_PART -1
#endif
#define MDQ_IN_PART(k) (MDQ_IPCS_PART == (k) || MDQ_IPCS_PART == -1)

#ifndef MDQ_SETUP_WG
#define MDQ_SETUP_WG 768
#endif
namespace mdq {

static __constant__ RefTab c_tab;

constexpr int MF_CH = 1024;  // triangles per LDS tile: 2 per thread, interleaved for FP64 ILP (host maps use the same chunking)

// ------------------------------------------------------------------ per-environment views

// mode 7: bytes that say which rows a workgroup's chunks touch, and which entries of the chunks' row lists are the FIRST
// touch of their row by that workgroup (a chunk's list holds at most min(N2, 6 MF_CH) rows), in doubles
__host__ __device__ inline int64_t work_touch_row_cap(int NV, int NE) {
  const int64_t N2 = (int64_t)NV + NE;
  return N2 < 6 * 1024 ? N2 : 6 * 1024;
}
__host__ __device__ inline int64_t work_touch_doubles(int NV, int NT, int NE) {
  const int64_t N2 = (int64_t)NV + NE, nch = ((int64_t)NT + 1023) / 1024;
  return (2 * N2 + nch * work_touch_row_cap(NV, NE) + 7) / 8 + 2;
}
__host__ __device__ inline int64_t work_per_env(int NV, int NT, int NE) {
  const int64_t N2 = (int64_t)NV + NE;
  // escr 12*NT | 6 velocity vectors (double2[N2]) | p_new[NV] | 24 spare | assembled modes: 5 history vectors + counter |
  // mode 5: the accumulation vector of the tile application (double2[N2]) | mode 7: the second workgroup's accumulation vector
  // | mode 7: touched-row bytes of the two workgroups (2 N2) + first-touch bytes of every chunk's row list
  const int64_t n = 12 * (int64_t)NT + 12 * N2 + NV + 26 + 10 * N2 + 2 + 2 * N2 + 2 + 2 * N2 + 2 + work_touch_doubles(NV, NT, NE);
  return (n + 31) & ~(int64_t)31;  // keep every environment's slab 256-byte aligned
}
// offset (in doubles, even) of the tentative-velocity history of the assembled modes 0-2 inside an environment's slab
__host__ __device__ inline int64_t work_hist_offset(int NV, int NT, int NE) {
  const int64_t N2 = (int64_t)NV + NE;
  return (12 * (int64_t)NT + 12 * N2 + NV + 24 + 1) & ~(int64_t)1;
}

// offset (in doubles, even) of mode 5's accumulation vector (behind the history vectors and their counter); mode 7's second
// one follows it at + 2 N2 + 2
__host__ __device__ inline int64_t work_ytmp_offset(int NV, int NT, int NE) {
  const int64_t N2 = (int64_t)NV + NE;
  return (work_hist_offset(NV, NT, NE) + 10 * N2 + 2 + 1) & ~(int64_t)1;
}

// offset (in doubles) of mode 7's touch bytes: behind the second accumulation vector
__host__ __device__ inline int64_t work_touch_offset(int NV, int NT, int NE) {
  const int64_t N2 = (int64_t)NV + NE;
  return work_ytmp_offset(NV, NT, NE) + 4 * N2 + 4;
}

// mode 5 with the chunk's input rows staged in LDS behind the element tile: does the stage (NRL rows) fit?
__host__ __device__ inline bool mode5_stage_fits(int NRL) {
  return NRL > 0 && 64 * sizeof(double) + sizeof(double2) * 6 * MF_CH + sizeof(double2) * (size_t)NRL <= 160 * 1024;
}
// LDS of the tile modes 5 / 7 behind the reduction scratch: the element tile (+ the stage of a chunk's input rows behind it when
// the packed local maps are given and fit) - what the launcher allocates and what the kernels may re-use in the pressure phase
__host__ __device__ inline size_t tile_lds_bytes(const mdq_ipcs_desc& d) {
  return sizeof(double2) * 6 * MF_CH +
         ((d.mf_lpos && d.mf_rlist && d.mf_rcnt && mode5_stage_fits(d.NRL)) ? sizeof(double2) * (size_t)d.NRL : 0);
}

struct EnvView {
  int nv, nt, ne, n2, nnz2, nnz1, naf;
  double mu, rho, dt;  // flow constants of THIS environment (the descriptor's scalars, or its row of env_phys)
  int NT;  // capacity (SoA stride of cell_dofs / geom)
  const double* coords;
  const int32_t* cell_dofs;  // [6][NT]
  const int8_t* cell_outflow;
  const int32_t *rowptr2, *colidx2, *asm2_ptr, *asm2_src;
  const int32_t *rowptr1, *colidx1, *asm1_ptr, *asm1_src;
  const int32_t *sl2_off, *sl2_col, *sl1_off, *sl1_col;
  const int32_t *mf_scat, *mf_tptr;
  int mf_tstride;  // N2+1
  const int32_t *mf_rlist, *mf_rcnt;   // mode 5: touched rows per chunk (or null)
  const int32_t* mf_lpos;              // mode 5: [6][NT] position of the dof in its chunk's row list | tile position << 16 (or null)
  int NRL, rl_flags;
  bool tiles;                          // modes 5 / 7: tile maps present (else: element scratch + dof <- slot lists)
  const int32_t *g2_ptr, *g2_src, *g1_ptr, *g1_src;
  const uint8_t* bcu_flag;
  const double* bcu_gx;
  const uint8_t* bcp_flag;
  const int32_t* af_facets;
  int nbo;
  const int32_t *bo_rows, *bo_ptr, *bo_col, *bo_src;
  double* bo_val;
  double* geom;  // [5][NT]
  double* A1;    // SELL [entries][4]
  double* Ms;
  double* K1s;
  double2* lift1;
  double2* lift3;
  double2* idiag1;
  double* sdiagM;
  double* sdiagK;
  double2* u_n;
  double* p_n;
  double* work;
#ifdef MDQ_PROFILE
  long long* sprof;  // LDS [8]: tile_accumulate phase cycles (thread 0)
#endif
};

// a workgroup-uniform double moved to scalar registers (two v_readfirstlane): loop invariants such as rho / dt, mu or the
// squared tolerance otherwise occupy a VGPR pair each for the whole Krylov loop (the 768-thread velocity kernel, capped at
// 168 VGPRs, spilled two of them and re-read them in every iteration)
__device__ __forceinline__ double uniform_double(double x) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll)), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Inflow schedule (mdq_ipcs_evolve_inflow): the factor a_b of environment b at step `step` of a launch of `nsteps`, table
// [B][nsteps] laid out like drag / lift.  Every velocity boundary condition but the inlet is zero and the symmetric
// elimination is linear in the Dirichlet vector, so a(t) * parabola needs no new set-up: the factor multiplies every READ of
// bcu_gx, lift1 and lift3 in that step (right-hand sides, Dirichlet rows of the initial guesses, norms of the stopping tests)
// and no array is rewritten: the set-up kernels and what they wrote for a = 1 stay as they are.  One uniform 8-byte load per
// workgroup and step, kept in scalar registers.  Without a table the factor is the literal 1.0; a table of ones gives the same
// bits (x * 1.0 is exact, and so is a contraction of f - 1.0 * l).  The pressure lifting is zero: at_pressure_kernel and phase
// 2 of evolve_mf_kernel read none of the three arrays.
__device__ __forceinline__ double inflow_factor(const double* tab, int b, int nsteps, int step) {
  return tab ? uniform_double(tab[(int64_t)b * nsteps + step]) : 1.0;
}
// the row of environment b as a pointer kept in a VGPR pair, and the factor loaded per lane through it: for a kernel whose
// scalar registers are the scarce ones (evolve_kernel's instance with the pressure vectors in the slab)
__device__ __forceinline__ const double* inflow_row_lane(const double* tab, int b, int nsteps) {
  unsigned long long a = reinterpret_cast<unsigned long long>(tab ? tab + (int64_t)b * nsteps : nullptr);
  asm volatile("" : "+v"(a));
  return reinterpret_cast<const double*>(a);
}
__device__ __forceinline__ double2 scaled2(double a, double2 x) { return make_double2(a * x.x, a * x.y); }

__device__ __forceinline__ EnvView env_view(const mdq_ipcs_desc& d, int b) {
  EnvView v;
  // flow constants: the batch-wide scalars, or row b of env_phys [B][4] = mu, rho, dt, 0.  b is the same for the whole
  // workgroup, so the row is one uniform 32-byte load; the values go through uniform_double and stay in scalar registers
  // like the kernel arguments they replace.  rho / dt is formed by the kernels from the view in both cases: a table whose
  // rows equal the scalars gives the bits of env_phys = NULL.
  v.mu = d.mu;
  v.rho = d.rho;
  v.dt = d.dt;
  if (d.env_phys) {
    const double4 q = *reinterpret_cast<const double4*>(d.env_phys + 4 * (int64_t)b);
    v.mu = uniform_double(q.x);
    v.rho = uniform_double(q.y);
    v.dt = uniform_double(q.z);
  }
  v.nv = d.nv[b];
  v.nt = d.nt[b];
  v.ne = d.ne[b];
  v.n2 = v.nv + v.ne;
  v.naf = d.naf[b];
  v.NT = d.NT;
  const int64_t B = b;
  v.coords = d.coords + B * d.NV * 2;
  v.cell_dofs = d.cell_dofs + B * 6 * d.NT;
  v.cell_outflow = d.cell_outflow + B * d.NT;
  v.rowptr2 = d.rowptr2 + B * (d.N2 + 1);
  v.colidx2 = d.colidx2 + B * d.NNZ2;
  v.asm2_ptr = d.asm2_ptr + B * (d.NNZ2 + 1);
  v.asm2_src = d.asm2_src + B * 36 * d.NT;
  v.rowptr1 = d.rowptr1 + B * (d.NV + 1);
  v.colidx1 = d.colidx1 + B * d.NNZ1;
  v.asm1_ptr = d.asm1_ptr + B * (d.NNZ1 + 1);
  v.asm1_src = d.asm1_src + B * 9 * d.NT;
  v.sl2_off = d.sl2_off + B * (d.N2 / 64 + 2);
  v.sl2_col = d.sl2_col + B * d.NSE2;
  v.sl1_off = d.sl1_off + B * (d.NV / 64 + 2);
  v.sl1_col = d.sl1_col + B * d.NSE1;
  v.mf_scat = d.mf_scat + B * 6 * d.NT;
  v.mf_tstride = d.N2 + 1;
  v.mf_tptr = d.mf_tptr ? d.mf_tptr + B * ((d.NT + MF_CH - 1) / MF_CH) * (d.N2 + 1) : nullptr;
  v.NRL = d.NRL;
  v.rl_flags = d.rl_flags;
  v.mf_rlist = (d.mf_rlist && d.mf_rcnt && d.NRL > 0) ? d.mf_rlist + B * ((d.NT + MF_CH - 1) / MF_CH) * d.NRL * 2 : nullptr;
  v.mf_rcnt = v.mf_rlist ? d.mf_rcnt + B * ((d.NT + MF_CH - 1) / MF_CH) : nullptr;
  // (maps built on the device, mdq_ipcs_build_tile_maps: a first count < 0 marks an environment whose maps could not be built -
  //  it keeps the dof <- slot path)
  if (v.mf_rcnt && !d.mf_tptr && v.mf_rcnt[0] < 0) v.mf_rlist = v.mf_rcnt = nullptr;
  v.mf_lpos = (v.mf_rlist && d.mf_lpos && mode5_stage_fits(d.NRL)) ? d.mf_lpos + B * 6 * d.NT : nullptr;
  // the element results of an operator application go through the LDS tile: host-built maps (mf_scat + mf_tptr; the row lists
  // optional) or the row lists + packed local maps alone (what the device builds)
  v.tiles = v.mf_tptr != nullptr || (v.mf_rlist != nullptr && v.mf_lpos != nullptr);
  v.g2_ptr = d.g2_ptr + B * (d.N2 + 1);
  v.g2_src = d.g2_src + B * 6 * d.NT;
  v.g1_ptr = d.g1_ptr + B * (d.NV + 1);
  v.g1_src = d.g1_src + B * 3 * d.NT;
  v.bcu_flag = d.bcu_flag + B * d.N2;
  v.bcu_gx = d.bcu_gx + B * d.N2;
  v.bcp_flag = d.bcp_flag + B * d.NV;
  v.af_facets = d.af_facets + B * d.NAF * 2;
  v.nbo = d.nbo ? d.nbo[b] : 0;
  v.bo_rows = d.bo_rows + B * d.NBO;
  v.bo_ptr = d.bo_ptr + B * (d.NBO + 1);
  v.bo_col = d.bo_col + B * d.NBE;
  v.bo_src = d.bo_src + B * d.NBE;
  v.bo_val = d.bo_val + B * d.NBE * 4;
  v.geom = d.geom + B * 5 * d.NT;
  v.A1 = d.A1 + B * d.NSE2 * 4;
  v.Ms = d.Ms + B * d.NSE2;
  v.K1s = d.K1s + B * d.NSE1;
  v.lift1 = reinterpret_cast<double2*>(d.lift1) + B * d.N2;
  v.lift3 = reinterpret_cast<double2*>(d.lift3) + B * d.N2;
  v.idiag1 = reinterpret_cast<double2*>(d.idiag1) + B * d.N2;
  v.sdiagM = d.sdiagM + B * d.N2;
  v.sdiagK = d.sdiagK + B * d.NV;
  v.u_n = reinterpret_cast<double2*>(d.u_n) + B * d.N2;
  v.p_n = d.p_n + B * d.NV;
  v.work = d.work + B * work_per_env(d.NV, d.NT, d.NE);
  v.nnz2 = v.nnz1 = 0;  // (filled by the assembly kernel: light descriptors carry no patterns)
  return v;
}

__device__ __forceinline__ Geo load_geo(const EnvView& v, int e) {
  Geo g;
  g.j00 = v.geom[0 * v.NT + e];
  g.j01 = v.geom[1 * v.NT + e];
  g.j10 = v.geom[2 * v.NT + e];
  g.j11 = v.geom[3 * v.NT + e];
  g.det = v.geom[4 * v.NT + e];
  return g;
}

__device__ __forceinline__ void load_cell_coords(const EnvView& v, int e, double (&X)[3][2]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int vid = v.cell_dofs[k * v.NT + e];
    X[k][0] = v.coords[2 * vid];
    X[k][1] = v.coords[2 * vid + 1];
  }
}

// single basis function / gradient at a reference point without register arrays
__device__ __forceinline__ double p2_phi_one(int i, double l0, double l1, double l2) {
  if (i < 3) {
    const double l = sel3(i, l0, l1, l2);
    return l * (2.0 * l - 1.0);
  }
  const int k = i - 3;
  return 4.0 * sel3(k, l1, l0, l0) * sel3(k, l2, l2, l1);
}

__device__ __forceinline__ void p2_dphi_one(int j, double l0, double l1, double l2, double& dx, double& dy) {
  // reference gradients of the barycentric coordinates
  if (j < 3) {
    const double f = 4.0 * sel3(j, l0, l1, l2) - 1.0;
    dx = f * sel3(j, -1.0, 1.0, 0.0);
    dy = f * sel3(j, -1.0, 0.0, 1.0);
    return;
  }
  const int k = j - 3;
  const double la = sel3(k, l1, l0, l0), lb = sel3(k, l2, l2, l1);
  const double dax = sel3(k, 1.0, -1.0, -1.0), day = sel3(k, 0.0, -1.0, -1.0);
  const double dbx = sel3(k, 0.0, 0.0, 1.0), dby = sel3(k, 1.0, 1.0, 0.0);
  dx = 4.0 * (la * dbx + lb * dax);
  dy = 4.0 * (la * dby + lb * day);
}

#if MDQ_IN_PART(0)
}  // namespace mdq
#include "mdq_ipcs_setup.hip"
namespace mdq {
#endif

// ================================================================== element right-hand sides

struct ElemIdx {
  int dof[6];
};

__device__ __forceinline__ ElemIdx load_dofs(const EnvView& v, int e) {
  ElemIdx E;
#pragma unroll
  for (int i = 0; i < 6; ++i) E.dof[i] = v.cell_dofs[i * v.NT + e];
  return E;
}

// element loops of the three right-hand sides: one thread per triangle, results to the
// per-environment scratch (slot = cell*6+i / cell*3+j) that the dof-gather passes read.  (first, stride): the triangles of
// this thread - the workgroup's by default, the team's in the two-workgroup kernels.  a = rho / dt and mu come from the
// caller, which knows where it keeps them (scalar registers; see uniform_double).
__device__ inline void rhs1_elements(const EnvView& v, const mdq_ipcs_desc& d, const double2* __restrict__ u,
                                     const double* __restrict__ p, double2* __restrict__ escr, double a, double mu,
                                     int first = threadIdx.x, int stride = WG) {
  for (int e = first; e < v.nt; e += stride) {
    const ElemIdx E = load_dofs(v, e);
    const Geo g = load_geo(v, e);
    double2 ue[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) ue[i] = u[E.dof[i]];
    double pe[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pe[i] = p[E.dof[i]];
    double2 r[6];
    elem_rhs1_vol(g, a, mu, v.rho, ue, pe, r);
    const int ko = v.cell_outflow[e];
    if (ko >= 0) {
      double X[3][2];
      load_cell_coords(v, e, X);
      elem_outflow_add(g, X, ko, 0.5 * mu, ue, r);  // + mu/2 <nabla_grad(u_n) n, v>
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) escr[e * 6 + i] = r[i];
  }
}

template <int NTH = WG>
__device__ inline void rhs2_elements(const EnvView& v, const mdq_ipcs_desc& d, const double2* __restrict__ u,
                                     const double* __restrict__ p, double* __restrict__ escr, int first = threadIdx.x,
                                     int stride = NTH) {
  const double idt = 1.0 / v.dt;
  for (int e = first; e < v.nt; e += stride) {
    const ElemIdx E = load_dofs(v, e);
    const Geo g = load_geo(v, e);
    double2 ue[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) ue[i] = u[E.dof[i]];
    double pe[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pe[i] = p[E.dof[i]];
    double r[3];
    elem_rhs2(g, idt, ue, pe, r);
#pragma unroll
    for (int j = 0; j < 3; ++j) escr[e * 3 + j] = r[j];
  }
}

// The same right-hand side accumulated straight into an LDS vector with fp64 LDS atomics (mode 3): no element
// scratch in global memory and no per-row gather lists (a dependent chain of three global round trips per row and
// one more per incident cell: 36 % of the direct pressure kernel).  Two triangles per thread, their loads issued
// together.  `acc` must be zeroed and published by the caller.
template <int NTH>
__device__ inline void rhs2_accumulate_lds(const EnvView& v, const mdq_ipcs_desc& d, const double2* __restrict__ u,
                                           const double* __restrict__ p, double* acc) {
  const double idt = 1.0 / v.dt;
  for (int e0 = threadIdx.x; e0 < v.nt; e0 += 2 * NTH) {
    const int e1 = e0 + NTH;
    const bool two = e1 < v.nt;
    const int ec = two ? e1 : e0;   // (clamped: the second triangle's loads are always issued)
    const ElemIdx Ea = load_dofs(v, e0), Eb = load_dofs(v, ec);
    const Geo ga = load_geo(v, e0), gb = load_geo(v, ec);
    double2 ua[6], ub[6];
    double pa[3], pb[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      ua[i] = u[Ea.dof[i]];
      ub[i] = u[Eb.dof[i]];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      pa[i] = p[Ea.dof[i]];
      pb[i] = p[Eb.dof[i]];
    }
    double ra[3], rb[3];
    elem_rhs2(ga, idt, ua, pa, ra);
    elem_rhs2(gb, idt, ub, pb, rb);
#pragma unroll
    for (int j = 0; j < 3; ++j) unsafeAtomicAdd(acc + Ea.dof[j], ra[j]);
    if (two) {
#pragma unroll
      for (int j = 0; j < 3; ++j) unsafeAtomicAdd(acc + Eb.dof[j], rb[j]);
    }
  }
}

__device__ inline void rhs3_elements(const EnvView& v, const mdq_ipcs_desc& d, const double2* __restrict__ u,
                                     const double* __restrict__ pnew, const double* __restrict__ pold,
                                     double2* __restrict__ escr, int first = threadIdx.x, int stride = WG) {
  for (int e = first; e < v.nt; e += stride) {
    const ElemIdx E = load_dofs(v, e);
    const Geo g = load_geo(v, e);
    double2 ue[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) ue[i] = u[E.dof[i]];
    double dp[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) dp[i] = pnew[E.dof[i]] - pold[E.dof[i]];
    double2 r[6];
    elem_rhs3(g, v.dt, ue, dp, r);
#pragma unroll
    for (int i = 0; i < 6; ++i) escr[e * 6 + i] = r[i];
  }
}

// ================================================================== matrix-free operator application
//
// y = Op x with the operator applied triangle by triangle (LDS-staged element tiles):
//   x   : gather vector in LDS (double2[n2])
//   es  : LDS tile of element results, SoA  es[i*CH + t]  (t = thread = triangle of the chunk)
// Per chunk of CH = WG triangles: every thread applies its triangle's 12x12 operator, barrier,
// then every thread sums the tile entries of its OWN rows (rows tid, tid+WG, ...) in ascending
// triangle order (fixed order => bitwise reproducible, no atomics), barrier.
// Requires n2 <= MF_ROWS*WG.
constexpr int MF_ROWS = 7;                     // own rows per thread: n2 <= MF_ROWS*WG = 3584

// Per-thread metadata of the triangles it applies in one chunk (MF_EPT = MF_CH / WG of them):
// 6 packed words (dof | tile position << 12 | (outflow edge + 1) << 28) + affine geometry.
// It is PREFETCHED one chunk ahead (rolling over to chunk 0 of the next application) so that the
// L2 latency of these loads hides behind the barrier / row-gather phase.
constexpr int MF_EPT = MF_CH / WG;
struct TileMeta {
  int w[MF_EPT][6];
  Geo g[MF_EPT];
};

__device__ __forceinline__ void tile_prefetch(const EnvView& v, TileMeta& tm, int chunk) {
#pragma unroll
  for (int j = 0; j < MF_EPT; ++j) {
    const int e = chunk * MF_CH + threadIdx.x + j * WG;
    if (e < v.nt) {
#pragma unroll
      for (int i = 0; i < 6; ++i) tm.w[j][i] = v.mf_scat[i * v.NT + e];
      tm.g[j] = load_geo(v, e);
    }
  }
}

// acc[k] = sum of the element results that land on own row tid + k*WG (zero for rows >= n2).
// op(e, geo, dofs, outflow_edge, ye) fills the 6 double2 results of triangle e.
// On entry tm holds the metadata of chunk 0; on exit again (prefetched for the next application).
template <class ElemOp>
__device__ __forceinline__ void tile_accumulate(const EnvView& v, double2* es, TileMeta& tm, ElemOp op,
                                                double2 (&acc)[MF_ROWS]) {
  const int tid = threadIdx.x, n = v.n2;
#pragma unroll
  for (int k = 0; k < MF_ROWS; ++k) acc[k] = make_double2(0.0, 0.0);
  const int nch = (v.nt + MF_CH - 1) / MF_CH;
#ifdef MDQ_PROFILE
  long long tq = __builtin_amdgcn_s_memtime();
#define MDQ_TSTAMP(k) { long long tn = __builtin_amdgcn_s_memtime(); if (tid == 0) v.sprof[k] += tn - tq; tq = tn; }
#else
#define MDQ_TSTAMP(k)
#endif
  for (int chunk = 0; chunk < nch; ++chunk) {
    double2* eb = es;
    // tile ranges of the own rows for this chunk (latency hides behind the element work)
    const int32_t* tp = v.mf_tptr + chunk * v.mf_tstride;
    int lohi[MF_ROWS];  // lo | hi << 16 (tile positions < 6*MF_CH < 65536)
#pragma unroll
    for (int k = 0; k < MF_ROWS; ++k) {
      const int row = tid + k * WG;
      lohi[k] = row < n ? (tp[row] | (tp[row + 1] << 16)) : 0;
    }
#pragma unroll
    for (int j = 0; j < MF_EPT; ++j) {
      const int e = chunk * MF_CH + tid + j * WG;
      if (e < v.nt) {
        ElemIdx E;
#pragma unroll
        for (int i = 0; i < 6; ++i) E.dof[i] = tm.w[j][i] & 0xFFF;
        double2 ye[6];
        op(e, tm.g[j], E, ((tm.w[j][0] >> 28) & 3) - 1, ye);
#pragma unroll
        for (int i = 0; i < 6; ++i) eb[(tm.w[j][i] >> 12) & 0x1FFF] = ye[i];
      }
    }
    MDQ_TSTAMP(0)
    tile_prefetch(v, tm, chunk + 1 < nch ? chunk + 1 : 0);
    MDQ_TSTAMP(1)
    __syncthreads();
    MDQ_TSTAMP(2)
#pragma unroll
    for (int k = 0; k < MF_ROWS; ++k) {
      for (int j = lohi[k] & 0xFFFF; j < (lohi[k] >> 16); ++j) {
        const double2 c = eb[j];
        acc[k].x += c.x;
        acc[k].y += c.y;
      }
    }
    MDQ_TSTAMP(3)
    __syncthreads();
    MDQ_TSTAMP(4)
  }
}

// MODE 5: the same element tiles for meshes whose vectors do not fit the LDS (ys930 red-refined: 12.9 k velocity dofs,
// 207 KB per vector): the operator input is gathered from GLOBAL memory (L2), the element results of a chunk go through the
// LDS tile, and the row owners (rows tid, tid + WG, ... as in every vector pass) add their tile entries - in fixed order -
// to an accumulation vector in the environment's workspace slab; after the last chunk every row hands its sum to `epi`.
// Per application and triangle: 6 dof ids + 6 tile positions + 5 geometry doubles + the outflow tag (89 B) instead of the
// 36 B per SELL entry of the assembled operator (~2 KB per triangle), and no sparsity pattern: like mode 2 it needs only
// what mdq_ipcs_setup_matfree derives on the device.  Bitwise reproducible.  mf_scat: packed words (N2 <= 4096) or plain
// tile positions (larger meshes, MeshTopology.matfree_maps).
#ifdef MDQ_T5_TRACE
// debug build only: s_memtime cycles of the phases of a mode-5 operator application (thread 0 of environment 0)
static __device__ long long mdq_t5_trace_buf[8];
#define T5_STAMP(k) { const long long tn_ = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0 && blockIdx.x == 0) mdq_t5_trace_buf[k] += tn_ - t5q_; t5q_ = tn_; }
#if MDQ_IN_PART(2)
extern "C" MDQ_API int mdq_t5_trace_host(long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mdq_t5_trace_buf), sizeof(long long) * 8) != hipSuccess) return -1;
  if (reset) { long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(mdq_t5_trace_buf), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
#endif
#else
#define T5_STAMP(k)
#endif

// The chunk loop of a tile application: chunks c0, c0 + cs, ... of the environment's triangles, their row sums accumulated
// into `ytmp` (c0 = 0, cs = 1: the whole operator; mode 7 deals the chunks out to the workgroups of a team, one accumulation
// vector each).  `flags_ok`: the touched-row lists mark the first chunk of every row IN THE ORDER 0, 1, 2, ... - usable only
// when this call walks all chunks in that order; otherwise the vector is zero-filled first.
template <class ElemOp>
__device__ __forceinline__ void tile_chunks_global(const EnvView& v, bool packed, double2* es, double2* ytmp, const double2* gx,
                                                   ElemOp op, int c0, int cs, bool flags_ok,
                                                   const unsigned char* firstb = nullptr, int first_stride = 0) {
  const int tid = threadIdx.x, n = v.n2;
  const int nch = (v.nt + MF_CH - 1) / MF_CH;
#ifdef MDQ_T5_TRACE
  long long t5q_ = __builtin_amdgcn_s_memtime();
  if (tid == 0 && blockIdx.x == 0) mdq_t5_trace_buf[7] += 1;
#endif
  // rl_flags: the touched-row lists mark the first / last chunk of every row - no zero fill and no read at the first touch
  // (9.29 -> 9.07 ms per step of 128 refined meshes).  Running the caller's epilogue at the LAST touch and dropping the pass
  // over the rows at the end (two more vector streams saved) was measured SLOWER, 10.52 ms: the epilogue's own loads then
  // sit one row at a time inside the row loop instead of four rows in flight
  const bool rlf = flags_ok && v.mf_rlist && v.rl_flags != 0;
  // (firstb, mode 7: first-touch bytes of THIS walk's chunks - one per entry of a chunk's row list, see team_touch_setup)
  const bool fb = firstb != nullptr && v.mf_rlist;
  if (!rlf && !fb)
    for (int row = tid; row < n; row += WG) ytmp[row] = make_double2(0.0, 0.0);   // (own rows: visible to the row phases behind the barriers)
  double2* xst = es + 6 * MF_CH;                        // (staged input rows of the chunk: behind the tile, mf_lpos only)
  for (int chunk = c0; chunk < nch; chunk += cs) {
    if (v.mf_lpos) {
      const int2* rl = reinterpret_cast<const int2*>(v.mf_rlist) + (size_t)chunk * v.NRL;
      const int nr = v.mf_rcnt[chunk];
      for (int k = tid; k < nr; k += WG) xst[k] = gx[rl[k].x & 0x3FFFFFFF];
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < MF_EPT; ++j) {
      const int e = chunk * MF_CH + tid + j * WG;
      if (e < v.nt) {
        int pos[6];
        double2 xe[6];
        if (v.mf_lpos) {
          int w[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) w[i] = v.mf_lpos[i * v.NT + e];
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            pos[i] = w[i] >> 16;
            xe[i] = xst[w[i] & 0xFFFF];
          }
        } else {
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            const int w = v.mf_scat[i * v.NT + e];
            pos[i] = packed ? (w >> 12) & 0x1FFF : w;
            xe[i] = gx[v.cell_dofs[i * v.NT + e]];
          }
        }
        const Geo g = load_geo(v, e);
        double2 ye[6];
        op(e, g, (int)v.cell_outflow[e], xe, ye);
#pragma unroll
        for (int i = 0; i < 6; ++i) es[pos[i]] = ye[i];
      }
    }
    T5_STAMP(0)
    __syncthreads();
    T5_STAMP(1)
    if (v.mf_rlist) {
      // row phase over the rows this chunk TOUCHES (ascending list: one thread per entry, a row belongs to one entry per
      // chunk): entry and running sum of a batch are requested together.  Walking every own row's tile range (the branch
      // below) visited 12 924 rows per chunk on the refined mesh for ~2 500 touched ones: 57 % of an application.
      const int2* rl = reinterpret_cast<const int2*>(v.mf_rlist) + (size_t)chunk * v.NRL;
      const int nr = v.mf_rcnt[chunk];
#ifndef MDQ_T5_RB
#define MDQ_T5_RB 8
#endif
      constexpr int RB = MDQ_T5_RB;
      for (int k0 = tid; k0 < nr; k0 += RB * WG) {
        int2 en[RB];
        double2 a[RB];
        unsigned fmask = 0;
#pragma unroll
        for (int k = 0; k < RB; ++k) en[k] = rl[min(k0 + k * WG, nr - 1)];
        if (fb) {
          const unsigned char* fbc = firstb + (size_t)chunk * first_stride;
#pragma unroll
          for (int k = 0; k < RB; ++k) fmask |= fbc[min(k0 + k * WG, nr - 1)] ? 1u << k : 0u;
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          a[k] = make_double2(0.0, 0.0);
          if (!((rlf && en[k].x < 0) || ((fmask >> k) & 1u))) a[k] = ytmp[en[k].x & 0x3FFFFFFF];
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          if (k0 + k * WG < nr) {
            const int lo = en[k].y & 0xFFFF, cnt = en[k].y >> 16, row = en[k].x & 0x3FFFFFFF;
            for (int j = lo; j < lo + cnt; ++j) {
              const double2 c = es[j];
              a[k].x += c.x;
              a[k].y += c.y;
            }
            ytmp[row] = a[k];
          }
        }
      }
    } else {
      // row phase in batches of RB own rows: the tile ranges and the running sums of a batch are requested together
      const int32_t* tp = v.mf_tptr + chunk * v.mf_tstride;
      constexpr int RB = 8;
      for (int row0 = tid; row0 < n; row0 += RB * WG) {
        int lo[RB], hi[RB];
        double2 a[RB];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          const int rc = min(row0 + k * WG, n - 1);
          lo[k] = tp[rc];
          hi[k] = tp[rc + 1];
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) a[k] = ytmp[min(row0 + k * WG, n - 1)];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          const int row = row0 + k * WG;
          if (row < n && hi[k] > lo[k]) {
            for (int j = lo[k]; j < hi[k]; ++j) {
              const double2 c = es[j];
              a[k].x += c.x;
              a[k].y += c.y;
            }
            ytmp[row] = a[k];
          }
        }
      }
    }
    T5_STAMP(2)
    __syncthreads();
    T5_STAMP(3)
  }
}

// `gx`: the operator's input vector (global); op(e, geometry, outflow edge, xe[6], ye[6]) applies one triangle's operator to
// its six gathered input values.  With mf_lpos (round 5) the rows a chunk touches are STAGED in LDS behind the tile first -
// one pass over the chunk's ascending row list, coalesced where the rows are consecutive - and the triangles gather from
// there through 16-bit local indices (the triangle's dof ids + tile positions are one packed word per dof: 24 B per
// triangle instead of 48).
template <class ElemOp, class Epi>
__device__ __forceinline__ void tile_apply_global(const EnvView& v, bool packed, double2* es, double2* ytmp, const double2* gx,
                                                  ElemOp op, Epi epi) {
  const int tid = threadIdx.x, n = v.n2;
  if (!v.tiles) {
    // no tile maps (index data built ON THE DEVICE by mdq_env_topology's large-mesh instance, which emits the dof <-
    // element-slot lists but no tile positions): the element results go to the slab's element scratch (6 double2 per
    // triangle, free during the solves) and every row sums its slots in ascending order - the gather the right-hand sides use
    double2* es2 = reinterpret_cast<double2*>(v.work);
    for (int e = tid; e < v.nt; e += WG) {
      double2 xe[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) xe[i] = gx[v.cell_dofs[i * v.NT + e]];
      const Geo g = load_geo(v, e);
      double2 ye[6];
      op(e, g, (int)v.cell_outflow[e], xe, ye);
#pragma unroll
      for (int i = 0; i < 6; ++i) es2[e * 6 + i] = ye[i];
    }
    __syncthreads();
    for (int row = tid; row < n; row += WG) {
      double2 a = make_double2(0.0, 0.0);
      for (int s = v.g2_ptr[row]; s < v.g2_ptr[row + 1]; ++s) {
        const double2 c = es2[v.g2_src[s]];
        a.x += c.x;
        a.y += c.y;
      }
      epi(row, a.x, a.y);
    }
    __syncthreads();
    return;
  }
  tile_chunks_global(v, packed, es, ytmp, gx, op, 0, 1, true);
#ifdef MDQ_T5_TRACE
  long long t5q_ = __builtin_amdgcn_s_memtime();
#endif
  // epilogue: the sums of a batch of own rows are requested together (the caller's own loads follow row by row)
#ifndef MDQ_T5_EB
#define MDQ_T5_EB 8
#endif
  constexpr int EB = MDQ_T5_EB;
  for (int row0 = tid; row0 < n; row0 += EB * WG) {
    double2 a[EB];
#pragma unroll
    for (int k = 0; k < EB; ++k) a[k] = ytmp[min(row0 + k * WG, n - 1)];
#pragma unroll
    for (int k = 0; k < EB; ++k)
      if (row0 + k * WG < n) epi(row0 + k * WG, a[k].x, a[k].y);
  }
  T5_STAMP(4)
}

// ================================================================== sparse kernels (workgroup-wide)
//
// SELL-64, one thread per row: wave w owns slices w, w+NWAVE, ... (rows tid, tid+WG, ...), the
// same ownership as every `for (i = tid; i < n; i += WG)` vector pass, so a thread only ever
// reads/writes its own entries of the Krylov vectors; only the SpMV input vector is gathered.
// Matrix loads are perfectly coalesced (64 lanes x 32 B / 8 B contiguous per instruction).

template <class Epi>
__device__ __forceinline__ void spmv_sell_b2(const int32_t* __restrict__ sl_off, const int32_t* __restrict__ sl_col,
                                             const double* __restrict__ A, const double2* x, int n, Epi epi) {
  const int lane = threadIdx.x & 63;
  const int nsl = (n + 63) >> 6;
  const double4* __restrict__ A4 = reinterpret_cast<const double4*>(A);
  for (int s = threadIdx.x >> 6; s < nsl; s += NWAVE) {
    const int base = sl_off[s], w = (sl_off[s + 1] - base) >> 6;
    const double4* a = A4 + base + lane;
    const int32_t* c = sl_col + base + lane;
    double y0 = 0.0, y1 = 0.0;
#ifndef MDQ_SPMV_UNROLL
#define MDQ_SPMV_UNROLL 4
#endif
#pragma unroll MDQ_SPMV_UNROLL
    for (int j = 0; j < w; ++j) {
      const double4 av = a[j * 64];
      const double2 xv = x[c[j * 64]];
      y0 += av.x * xv.x + av.y * xv.y;
      y1 += av.z * xv.x + av.w * xv.y;
    }
    const int row = (s << 6) + lane;
    if (row < n) epi(row, y0, y1);
  }
}

template <class Epi>
__device__ __forceinline__ void spmv_sell_2rhs(const int32_t* __restrict__ sl_off, const int32_t* __restrict__ sl_col,
                                               const double* __restrict__ A, const double2* x, int n, Epi epi) {
  const int lane = threadIdx.x & 63;
  const int nsl = (n + 63) >> 6;
  for (int s = threadIdx.x >> 6; s < nsl; s += NWAVE) {
    const int base = sl_off[s], w = (sl_off[s + 1] - base) >> 6;
    const double* a = A + base + lane;
    const int32_t* c = sl_col + base + lane;
    double y0 = 0.0, y1 = 0.0;
#pragma unroll 4
    for (int j = 0; j < w; ++j) {
      const double av = a[j * 64];
      const double2 xv = x[c[j * 64]];
      y0 += av * xv.x;
      y1 += av * xv.y;
    }
    const int row = (s << 6) + lane;
    if (row < n) epi(row, y0, y1);
  }
}

template <class Epi>
__device__ __forceinline__ void spmv_sell(const int32_t* sl_off, const int32_t* sl_col, const double* A,
                                          const double* x, int n, Epi epi) {
  const int lane = threadIdx.x & 63;
  const int nsl = (n + 63) >> 6;
  for (int s = threadIdx.x >> 6; s < nsl; s += NWAVE) {
    const int base = sl_off[s], w = (sl_off[s + 1] - base) >> 6;
    const double* a = A + base + lane;
    const int32_t* c = sl_col + base + lane;
    double y0 = 0.0;
#pragma unroll 3
    for (int j = 0; j < w; ++j) y0 += a[j * 64] * x[c[j * 64]];
    const int row = (s << 6) + lane;
    if (row < n) epi(row, y0);
  }
}

// ================================================================== Krylov solvers
//
// MODE 0: assembled SELL operators, gather vectors in global memory (any mesh size)
// MODE 1: assembled SELL operators, gather vectors p / r resident in LDS
// MODE 5: element-tile operators (tile of element results in LDS, gather vectors in global memory)
//
// The three evolve kernels (one workgroup per environment, and the two team kernels further down) run the SAME solvers and
// the same row phases of the time step.  What differs between them is a ROW GROUP: which rows of a vector pass a thread
// walks, what the barrier between a producer and a consumer phase is, and how a sum over all rows is formed -
//   rows(n, f)       f(i) for the rows of this thread among 0 .. n
//   sync()           the barrier that separates a producer phase from a consumer phase
//   sum(acc, red)    the deterministic reduction; every thread of the group receives the same bits
// - and the operator application, a callable (const double2* gx, Epi epi) that gathers from gx and hands every row of the
// group to epi(row, y0, y1) once.  WgRows is one workgroup; TeamRows (behind `Team`) is the two workgroups of a team.
struct WgRows {
  template <class F>
  __device__ __forceinline__ void rows(int n, F f) const {
    for (int i = threadIdx.x; i < n; i += WG) f(i);
  }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  template <int N>
  __device__ __forceinline__ void sum(double (&acc)[N], double* red) const { block_sum<N>(acc, red); }
};

struct VelCtx {
  double2* x;    // solution (own rows)
  double2* r;    // residual / s (own rows); SpMV #2 gathers s from it
  double2* rh;   // shadow residual (own rows)
  double2* p;    // search direction (own rows); SpMV #1 gathers p from it
  double2* vv;   // A p (own rows)
  double2* t;    // A s (own rows)
  // read by apply_velocity<MODE> only:
  double2* es;   // MODE 5: LDS element tile
  double2* yt;   // MODE 5: accumulation vector (global, own rows)
  bool packed;   // MODE 5: mf_scat holds packed words
  double a, mu;
};

// y = (D^-1 A1_bc) x on vectors that vanish on constrained dofs (see bicgstab_velocity)
__device__ __forceinline__ void velocity_op(const EnvView& v, double a, double mu, int e, int ko, const Geo& g,
                                            const double2 (&xe)[6], double2 (&ye)[6]);

template <int MODE, class Epi>
__device__ __forceinline__ void apply_velocity(const EnvView& v, const VelCtx& c, const double2* gx, Epi epi) {
  static_assert(MODE != 2, "the LDS-resident matrix-free mode has its own kernel (evolve_mf_kernel)");
  if constexpr (MODE == 5) {
    // full element operator on the gathered vector, rows scaled by D^-1 (0 on constrained rows) on the way out
    tile_apply_global(
        v, c.packed, c.es, c.yt, gx,
        [&](int e, const Geo& g, int ko, const double2(&xe)[6], double2(&ye)[6]) { velocity_op(v, c.a, c.mu, e, ko, g, xe, ye); },
        [&](int row, double y0, double y1) {
          const bool fl = v.bcu_flag[row] != 0;
          const double2 id = v.idiag1[row];
          epi(row, fl ? 0.0 : y0 * id.x, fl ? 0.0 : y1 * id.y);
        });
  } else {
    spmv_sell_b2(v.sl2_off, v.sl2_col, v.A1, gx, v.n2, epi);
  }
}

// BiCGStab on the row-scaled velocity system  (D^-1 A1_bc) x = D^-1 b.
// Entry: c.r holds the initial residual r0 = D^-1 (b - A x0) (zero on constrained dofs because x0
// already satisfies the Dirichlet values), bb = |D^-1 b|^2 and rr0 = |r0|^2 are group-uniform.
// Every Krylov vector therefore vanishes on constrained dofs and the eliminated operator equals the
// plain element operator on them.  Exit: c.x holds the solution on the rows of their owners - the barrier that
// publishes it is the caller's (one barrier there, not two: a team barrier is a spin and cache maintenance).
// Every exit is group-uniform: it tests sums that every thread of the group holds with the same bits.
template <class RG, class Op>
__device__ __forceinline__ int bicgstab_velocity(const RG& rg, const Op& apply, const EnvView& v, const VelCtx& c, double rtol,
                                                 int maxit, double bb, double rr0, double* red) {
  const int n = v.n2;
  const double tol2 = rtol * rtol * bb;
  double rr = rr0;
  if (!(rr > tol2) || bb == 0.0) return 0;
  double rho = rr, rho_old = 1.0, alpha = 1.0, omega = 1.0;  // rh = r0, p = v = 0 on entry
  int it = 0;
  while (it < maxit) {
    ++it;
    const double beta = (rho / rho_old) * (alpha / omega);
    rg.rows(n, [&](int i) {
      const double2 ri = c.r[i], pi = c.p[i], vi = c.vv[i];
      c.p[i] = make_double2(ri.x + beta * (pi.x - omega * vi.x), ri.y + beta * (pi.y - omega * vi.y));
    });
    rg.sync();
    double a1[1] = {0.0};
    apply(c.p, [&](int row, double y0, double y1) {
      c.vv[row] = make_double2(y0, y1);
      const double2 h = c.rh[row];
      a1[0] += h.x * y0 + h.y * y1;
    });
    rg.sum(a1, red);
    if (a1[0] == 0.0) break;  // breakdown
    alpha = rho / a1[0];
    double a2[1] = {0.0};
    rg.rows(n, [&](int i) {
      const double2 ri = c.r[i], vi = c.vv[i];
      const double2 sv = make_double2(ri.x - alpha * vi.x, ri.y - alpha * vi.y);
      c.r[i] = sv;
      a2[0] += sv.x * sv.x + sv.y * sv.y;
    });
    rg.sum(a2, red);  // (its barriers also publish s)
    if (!(a2[0] > tol2)) {
      rg.rows(n, [&](int i) {
        const double2 xi = c.x[i], pi = c.p[i];
        c.x[i] = make_double2(xi.x + alpha * pi.x, xi.y + alpha * pi.y);
      });
      break;
    }
    double a3[2] = {0.0, 0.0};
    apply(c.r, [&](int row, double y0, double y1) {
      c.t[row] = make_double2(y0, y1);
      const double2 sv = c.r[row];
      a3[0] += y0 * sv.x + y1 * sv.y;
      a3[1] += y0 * y0 + y1 * y1;
    });
    rg.sum(a3, red);
    if (a3[1] == 0.0) break;
    omega = a3[0] / a3[1];
    double a4[2] = {0.0, 0.0};
    rg.rows(n, [&](int i) {
      const double2 ti = c.t[i], xi = c.x[i], pi = c.p[i], si = c.r[i], hi = c.rh[i];
      c.x[i] = make_double2(xi.x + alpha * pi.x + omega * si.x, xi.y + alpha * pi.y + omega * si.y);
      const double2 rn = make_double2(si.x - omega * ti.x, si.y - omega * ti.y);
      c.r[i] = rn;
      a4[0] += rn.x * rn.x + rn.y * rn.y;
      a4[1] += hi.x * rn.x + hi.y * rn.y;
    });
    rg.sum(a4, red);
    rr = a4[0];
    if (!(rr > tol2)) break;
    rho_old = rho;
    rho = a4[1];
    if (rho == 0.0 || omega == 0.0) break;
  }
  return it;
}

struct MassCtx {
  double2* x;   // S x (own rows)
  double2* r;   // residual (own rows)
  double2* p;   // search direction (own rows)
  double2* q;   // M p (own rows)
  double2* gp;  // where the SpMV gathers from: p itself, or (tile operators) the staged copy S^-1 p
  // read by apply_mass<MODE> only:
  double2* es;  // MODE 5: LDS element tile
  double2* yt;  // MODE 5: accumulation vector (global, own rows)
  bool packed;
};

// y = (S^-1 M_bc S^-1) x on vectors that vanish on constrained dofs
template <int MODE, class Epi>
__device__ __forceinline__ void apply_mass(const EnvView& v, const MassCtx& c, const double2* gx, Epi epi) {
  static_assert(MODE != 2, "the LDS-resident matrix-free mode has its own kernel (evolve_mf_kernel)");
  if constexpr (MODE == 5) {
    // gx holds S^-1 p (staged by the caller); rows scaled by S^-1 (0 on constrained rows) on the way out
    tile_apply_global(
        v, c.packed, c.es, c.yt, gx,
        [&](int, const Geo& g, int, const double2(&xe)[6], double2(&ye)[6]) { elem_mass(g, xe, ye); },
        [&](int row, double y0, double y1) {
          const double is = v.bcu_flag[row] ? 0.0 : 1.0 / v.sdiagM[row];
          epi(row, y0 * is, y1 * is);
        });
  } else {
    spmv_sell_2rhs(v.sl2_off, v.sl2_col, v.Ms, gx, v.n2, epi);
  }
}

// CG on the symmetrically scaled mass system, both velocity components at once.
// Entry: c.r = r0 = S^-1 (b - M S^-1 x0) with zeros on constrained dofs, c.p = r0 (and, STAGED, c.gp = S^-1 r0: the tile
// operators apply the plain element mass matrix to a gathered S^-1 p).  Exit: as bicgstab_velocity - no barrier.
template <bool STAGED, class RG, class Op>
__device__ __forceinline__ int cg_mass(const RG& rg, const Op& apply, const EnvView& v, const MassCtx& c, double rtol, int maxit,
                                       double bb, double rr0, double* red) {
  const int n = v.n2;
  const double tol2 = rtol * rtol * bb;
  double rr = rr0;
  if (!(rr > tol2) || bb == 0.0) return 0;
  int it = 0;
  while (it < maxit) {
    ++it;
    double a1[1] = {0.0};
    apply(c.gp, [&](int row, double y0, double y1) {
      c.q[row] = make_double2(y0, y1);
      const double2 pi = c.p[row];
      a1[0] += pi.x * y0 + pi.y * y1;
    });
    rg.sum(a1, red);
    if (!(a1[0] > 0.0)) break;
    const double alpha = rr / a1[0];
    double a2[1] = {0.0};
    rg.rows(n, [&](int i) {
      const double2 xi = c.x[i], pi = c.p[i], ri = c.r[i], qi = c.q[i];
      c.x[i] = make_double2(xi.x + alpha * pi.x, xi.y + alpha * pi.y);
      const double2 rn = make_double2(ri.x - alpha * qi.x, ri.y - alpha * qi.y);
      c.r[i] = rn;
      a2[0] += rn.x * rn.x + rn.y * rn.y;
    });
    rg.sum(a2, red);
    const double rr_new = a2[0];
    if (!(rr_new > tol2)) break;
    const double beta = rr_new / rr;
    rr = rr_new;
    rg.rows(n, [&](int i) {
      const double2 ri = c.r[i], pi = c.p[i];
      const double2 pn = make_double2(ri.x + beta * pi.x, ri.y + beta * pi.y);
      c.p[i] = pn;
      if (STAGED) {
        const double is = 1.0 / v.sdiagM[i];
        c.gp[i] = make_double2(pn.x * is, pn.y * is);
      }
    });
    rg.sync();
  }
  return it;
}

// CG on the symmetrically scaled pressure system; vectors (and, when it fits, the matrix) in LDS.
__device__ inline int cg_pressure(int n, const int32_t* sl_off, const int32_t* sl_col, const double* A, double rtol,
                                  int maxit, double* x, double* r, double* p, double* q, double* red) {
  const int tid = threadIdx.x;
  double acc[2] = {0.0, 0.0};
  __syncthreads();
  spmv_sell(sl_off, sl_col, A, x, n, [&](int row, double y0) {
    const double b = r[row];
    const double rr = b - y0;
    r[row] = rr;
    p[row] = rr;
    acc[0] += b * b;
    acc[1] += rr * rr;
  });
  block_sum<2>(acc, red);
  const double bb = acc[0];
  double rr = acc[1];
  const double tol2 = rtol * rtol * bb;
  if (!(rr > tol2) || bb == 0.0) return 0;
  int it = 0;
  while (it < maxit) {
    ++it;
    double a1[1] = {0.0};
    spmv_sell(sl_off, sl_col, A, p, n, [&](int row, double y0) {
      q[row] = y0;
      a1[0] += p[row] * y0;
    });
    block_sum<1>(a1, red);
    if (!(a1[0] > 0.0)) break;
    const double alpha = rr / a1[0];
    double a2[1] = {0.0};
    for (int i = tid; i < n; i += WG) {
      x[i] += alpha * p[i];
      const double rn = r[i] - alpha * q[i];
      r[i] = rn;
      a2[0] += rn * rn;
    }
    block_sum<1>(a2, red);
    const double rr_new = a2[0];
    if (!(rr_new > tol2)) break;
    const double beta = rr_new / rr;
    rr = rr_new;
    for (int i = tid; i < n; i += WG) p[i] = r[i] + beta * p[i];
    __syncthreads();
  }
  __syncthreads();
  return it;
}

// aggregates of the two-level preconditioners (cg_pressure_2l in mdq_ipcs_pcg_reg.hip; tl_build and its users below)
constexpr int NAGX = 8, NAGY = 7, NAG = NAGX * NAGY;
#if MDQ_IN_PART(0)
}  // namespace mdq
#include "mdq_ipcs_pcg_reg.hip"
namespace mdq {
#endif

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

#if MDQ_IN_PART(0)
static __global__ __launch_bounds__(WG) void probe_kernel(mdq_ipcs_desc d, int nfields, const double* u, const double* p,
                                                    double* drag, double* lift) {
  __shared__ double red[NWAVE * 2];
  const int b = blockIdx.x;
  const EnvView v = env_view(d, b);
  for (int f = 0; f < nfields; ++f) {
    const double2* uf = reinterpret_cast<const double2*>(u) + ((int64_t)b * nfields + f) * d.N2;
    const double* pf = p + ((int64_t)b * nfields + f) * d.NV;
    double dr, li;
    forces(v, v.mu, uf, pf, red, dr, li);
    if (threadIdx.x == 0) {
      drag[(int64_t)b * nfields + f] = dr;
      lift[(int64_t)b * nfields + f] = li;
    }
    __syncthreads();
  }
}
#endif

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
constexpr int TEAM = 2;
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

// "No initial-guess history on a new mesh" (FlowSolver.remesh restarts u_n / p_n and the solvers, flow_solver.py:233-359):
// the counters of the extrapolated initial guesses (tentative velocities stored, corrections stored / ring position / lagged
// |b| / step parity of the fused correction start), of every operator mode, back to zero - instead of a fill of the whole
// workspace (100 MB per 128 environments in every S3 env step) - and, optionally, the iteration counters.
#if MDQ_IN_PART(0)
static __global__ void reset_history_kernel(mdq_ipcs_desc d, int32_t* iters) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  double* w = d.work + (int64_t)b * work_per_env(d.NV, d.NT, d.NE);
  double2* xs = reinterpret_cast<double2*>(w + 12 * (int64_t)d.NT);
  reinterpret_cast<double*>(xs + 3 * (int64_t)d.N2)[0] = 0.0;                       // mode 3: histc
  double2* h1 = reinterpret_cast<double2*>(w + work_hist_offset(d.NV, d.NT, d.NE));
  double* ccnt = reinterpret_cast<double*>(h1 + 3 * (int64_t)d.N2);                  // mode 3: correction ring
  ccnt[0] = ccnt[1] = ccnt[2] = ccnt[3] = 0.0;
  reinterpret_cast<double*>(h1 + 5 * (int64_t)d.N2)[0] = 0.0;                        // modes 0-2, 4, 5: hcnt
  reinterpret_cast<double*>(h1 + 5 * (int64_t)d.N2)[1] = 0.0;                        // mode 2: corrections stored
  if (iters) iters[3 * b] = iters[3 * b + 1] = iters[3 * b + 2] = 0;
}
#endif

static __global__ void team_reset_kernel(mdq_ipcs_desc d);   // (defined in part 2 only; named by launch_evolve_team)
#if MDQ_IN_PART(2)
static __global__ void team_reset_kernel(mdq_ipcs_desc d) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  double* w = d.work + (int64_t)b * work_per_env(d.NV, d.NT, d.NE);
  double* spare = w + 12 * (int64_t)d.NT + 12 * (int64_t)d.N2 + d.NV;
  unsigned* ctr = reinterpret_cast<unsigned*>(spare + 8);
  ctr[0] = ctr[1] = 0u;
}
#endif

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

__device__ __forceinline__ void velocity_op(const EnvView& v, double a, double mu, int e, int ko, const Geo& g,
                                            const double2 (&xe)[6], double2 (&ye)[6]) {
  elem_velocity(g, a, mu, xe, ye);
  if (ko >= 0) {
    double X[3][2];
    load_cell_coords(v, e, X);
    elem_outflow_add(g, X, ko, -0.5 * mu, xe, ye);
  }
}

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

#if MDQ_IN_PART(0)
}  // namespace mdq
#include "mdq_ipcs_mode3.hip"
namespace mdq {
#endif


// ================================================================== host side

static void build_tables(RefTab& T) {
  const double s15 = std::sqrt(15.0);
  const double a1 = (6.0 - s15) / 21.0, a2 = (6.0 + s15) / 21.0;
  const double w0 = 9.0 / 40.0, w1 = (155.0 - s15) / 1200.0, w2 = (155.0 + s15) / 1200.0;
  const double pts[NQ][2] = {{1.0 / 3.0, 1.0 / 3.0}, {a1, a1}, {1.0 - 2.0 * a1, a1}, {a1, 1.0 - 2.0 * a1},
                             {a2, a2},               {1.0 - 2.0 * a2, a2}, {a2, 1.0 - 2.0 * a2}};
  const double wts[NQ] = {w0, w1, w1, w1, w2, w2, w2};
  auto basis = [](double xi, double eta, double* phi, double (*dphi)[2], double* psi) {
    const double lam[3] = {1.0 - xi - eta, xi, eta};
    const double dl[3][2] = {{-1.0, -1.0}, {1.0, 0.0}, {0.0, 1.0}};
    const int EA[3] = {1, 0, 0}, EB[3] = {2, 2, 1};
    for (int k = 0; k < 3; ++k) {
      psi[k] = lam[k];
      phi[k] = lam[k] * (2.0 * lam[k] - 1.0);
      dphi[k][0] = (4.0 * lam[k] - 1.0) * dl[k][0];
      dphi[k][1] = (4.0 * lam[k] - 1.0) * dl[k][1];
      phi[3 + k] = 4.0 * lam[EA[k]] * lam[EB[k]];
      dphi[3 + k][0] = 4.0 * (lam[EA[k]] * dl[EB[k]][0] + lam[EB[k]] * dl[EA[k]][0]);
      dphi[3 + k][1] = 4.0 * (lam[EA[k]] * dl[EB[k]][1] + lam[EB[k]] * dl[EA[k]][1]);
    }
  };
  std::memset(&T, 0, sizeof(T));
  for (int q = 0; q < NQ; ++q) {
    T.qw[q] = 0.5 * wts[q];
    basis(pts[q][0], pts[q][1], T.qphi[q], T.qdphi[q], T.qpsi[q]);
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) {
        T.Mhat[i][j] += T.qw[q] * T.qphi[q][i] * T.qphi[q][j];
        for (int c = 0; c < 2; ++c)
          for (int dd = 0; dd < 2; ++dd) T.Ghat[c][dd][i][j] += T.qw[q] * T.qdphi[q][i][c] * T.qdphi[q][j][dd];
      }
  }
  const double g = 0.5 / std::sqrt(3.0);
  T.gx[0] = 0.5 - g;
  T.gx[1] = 0.5 + g;
  T.gw[0] = T.gw[1] = 0.5;
}

// the reference-element tables of THIS translation unit's kernels (c_tab has internal linkage)
static hipError_t upload_tables() {
  static std::once_flag once;
  static hipError_t err = hipSuccess;
  std::call_once(once, [] {
    RefTab T;
    build_tables(T);
    err = hipMemcpyToSymbol(HIP_SYMBOL(c_tab), &T, sizeof(T));
  });
  return err;
}

#if MDQ_IN_PART(0)
}  // namespace mdq
#include "mdq_ipcs_inflow.hip"
namespace mdq {
#endif

// launchers of the operator modes whose kernels live in the other parts of this file (each uploads its own tables)
struct EvolveArgs {
  const mdq_ipcs_desc* d;
  size_t lds;
  int nsteps;
  double *drag, *lift;
  int32_t* iters;
  const double* inflow_scale;   // [B][nsteps] inflow factors, or null (mdq_ipcs_evolve_inflow)
  hipStream_t st;
  const mdq_inflow_profile* prof;   // inflow profile of the per-step mode 2, or null (mdq_ipcs_evolve_profile)
};
hipError_t part_launch_assembled(int mode, bool k1_lds, bool pg, const EvolveArgs& a);   // modes 0 / 1 (part 1)
hipError_t part_launch_tiles(int mode, bool k1_lds, bool pg, const EvolveArgs& a);       // modes 5 / 4 (part 2)
hipError_t part_launch_mf(bool k1_lds, const EvolveArgs& a);                              // mode 2     (part 3)

#if MDQ_IN_PART(1)
hipError_t part_launch_assembled(int mode, bool k1_lds, bool pg, const EvolveArgs& a) {
  if (hipError_t e = upload_tables(); e != hipSuccess) return e;
  if (mode == 1)
    return k1_lds ? launch_evolve<1, true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
                  : launch_evolve<1, false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st);
  return pg ? launch_evolve<0, false, true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
            : (k1_lds ? launch_evolve<0, true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
                      : launch_evolve<0, false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st));
}
#endif
#if MDQ_IN_PART(2)
hipError_t part_launch_tiles(int mode, bool k1_lds, bool pg, const EvolveArgs& a) {
  if (hipError_t e = upload_tables(); e != hipSuccess) return e;
  if (mode == 4)
    return k1_lds ? launch_evolve_team<true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
                  : launch_evolve_team<false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st);
  if (mode == 7)
    return k1_lds ? launch_evolve_team_tiles<true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
                  : launch_evolve_team_tiles<false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st);
  return pg ? launch_evolve<5, false, true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
            : (k1_lds ? launch_evolve<5, true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
                      : launch_evolve<5, false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st));
}
#endif
#if MDQ_IN_PART(3)
hipError_t part_launch_mf(bool k1_lds, const EvolveArgs& a) {
  if (hipError_t e = upload_tables(); e != hipSuccess) return e;
  return k1_lds ? launch_evolve_mf<true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.prof, a.st)
                : launch_evolve_mf<false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.prof, a.st);
}
#endif

}  // namespace mdq

#if MDQ_IN_PART(0)
#include "mdq_ipcs_entry.hip"
#endif
