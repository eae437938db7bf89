// Translation unit ipcs3: the matrix-free mode 2 (element tiles, LDS / register vectors) - evolve_mf_kernel and its launcher
// part_launch_mf.
#include "mdq_ipcs_views.hip"
#include "mdq_ipcs_ops.hip"
#include "mdq_ipcs_pressure.hip"
#include "mdq_ipcs_step.hip"
#include "mdq_ipcs_mf.hip"
#include "mdq_ipcs_tables.hip"
#include "mdq_ipcs_launch.hip"

namespace mdq {

hipError_t part_launch_mf(bool k1_lds, const EvolveArgs& a) {
  if (hipError_t e = upload_tables(); e != hipSuccess) return e;
  return k1_lds ? launch_evolve_mf<true>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.prof, a.st)
                : launch_evolve_mf<false>(a.d, a.lds, a.nsteps, a.drag, a.lift, a.iters, a.inflow_scale, a.prof, a.st);
}

}  // namespace mdq
