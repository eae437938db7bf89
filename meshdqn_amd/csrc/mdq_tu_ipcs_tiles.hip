// Translation unit ipcs2: element tiles with global vectors (mode 5) and the two-workgroup team kernels (modes 4 / 7) -
// evolve_kernel<5>, evolve_team_kernel, evolve_team_tiles_kernel and their launcher part_launch_tiles.
#include "mdq_ipcs_views.hip"
#include "mdq_ipcs_ops.hip"
#include "mdq_ipcs_pressure.hip"
#include "mdq_ipcs_step.hip"
#include "mdq_ipcs_evolve.hip"
#include "mdq_ipcs_team.hip"
#include "mdq_ipcs_tables.hip"
#include "mdq_ipcs_launch.hip"

namespace mdq {

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

}  // namespace mdq
