// Translation unit ipcs1: the assembled SELL operators, one workgroup per environment (modes 0 / 1) - evolve_kernel<0 / 1>
// and their launcher part_launch_assembled.
#include "mdq_ipcs_views.hip"
#include "mdq_ipcs_ops.hip"
#include "mdq_ipcs_pressure.hip"
#include "mdq_ipcs_step.hip"
#include "mdq_ipcs_evolve.hip"
#include "mdq_ipcs_tables.hip"
#include "mdq_ipcs_launch.hip"

namespace mdq {

hipError_t part_launch_assembled(int mode, bool k1_lds, bool pg, const EvolveArgs& a) {
  if (hipError_t e = upload_tables(); e != hipSuccess) return e;
  if (mode == 1)
    return k1_lds ? launch_evolve<1, true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
                  : launch_evolve<1, false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st);
  return pg ? launch_evolve<0, false, true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
            : (k1_lds ? launch_evolve<0, true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st)
                      : launch_evolve<0, false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.st));
}

}  // namespace mdq
