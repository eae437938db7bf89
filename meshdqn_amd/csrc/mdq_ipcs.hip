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

// The IPCS code is four translation units (meshdqn_amd/build.py: ipcs0 - ipcs3), each instantiating the kernels of some operator
// modes together with their launchers - as ONE unit it took a minute of every rebuild.  What the units share stands in
// fragments that all of them include (mdq_ipcs_views.hip, mdq_ipcs_ops.hip, mdq_ipcs_pressure.hip, mdq_ipcs_step.hip,
// mdq_ipcs_tables.hip, mdq_ipcs_launch.hip); a kernel family stands in ONE fragment, included by the units that instantiate it:
//   this file (ipcs0)          the entry unit: the probe kernel and the history reset here; assembly and the matrix-free
//           set-up (mdq_ipcs_setup.hip), the register-resident pressure solvers of mode 3 (mdq_ipcs_pcg_reg.hip), the three
//           kernels of mode 3 (mdq_ipcs_mode3.hip), the inflow profile and the inlet map (mdq_ipcs_inflow.hip), the error
//           state and the entry points with the launch sequence of mode 3 (mdq_ipcs_entry.hip)
//   mdq_tu_ipcs_assembled.hip  (ipcs1)  evolve_kernel<0 / 1> (mdq_ipcs_evolve.hip; assembled SELL operators)
//   mdq_tu_ipcs_tiles.hip      (ipcs2)  evolve_kernel<5> (element tiles, global vectors), evolve_team_kernel (mode 4) and
//           evolve_team_tiles_kernel (mode 7) (mdq_ipcs_team.hip)
//   mdq_tu_ipcs_mf.hip         (ipcs3)  the kernels of mode 2 (mdq_ipcs_mf.hip; element tiles, LDS / register vectors: the
//           reproducible mode of the long runs)
// ("part k" in a comment or a name - part_launch_tiles, "defined in part 0" - is unit ipcsk: the units were parts of this file.)
// Kernels and device tables have internal linkage: every unit owns a copy of the reference-element tables (upload_tables).

#ifndef MDQ_SETUP_WG
#define MDQ_SETUP_WG 768
#endif

#include "mdq_ipcs_views.hip"
#include "mdq_ipcs_setup.hip"
#include "mdq_ipcs_ops.hip"
#include "mdq_ipcs_pcg_reg.hip"
#include "mdq_ipcs_pressure.hip"
#include "mdq_ipcs_step.hip"

namespace mdq {

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

// "No initial-guess history on a new mesh" (FlowSolver.remesh restarts u_n / p_n and the solvers, flow_solver.py:233-359):
// the counters of the extrapolated initial guesses (tentative velocities stored, corrections stored / ring position / lagged
// |b| / step parity of the fused correction start), of every operator mode, back to zero - instead of a fill of the whole
// workspace (100 MB per 128 environments in every S3 env step) - and, optionally, the iteration counters.
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

}  // namespace mdq

#include "mdq_ipcs_mode3.hip"
#include "mdq_ipcs_tables.hip"
#include "mdq_ipcs_inflow.hip"
#include "mdq_ipcs_launch.hip"
#include "mdq_ipcs_entry.hip"
