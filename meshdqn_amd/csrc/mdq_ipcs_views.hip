// IPCS, shared: the headers, the layout of an environment's workspace slab, the per-environment views (EnvView, env_view),
// block sums and the geometry helpers.  Included by all four IPCS units, first.
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

}  // namespace mdq
