// IPCS, shared: what the units know of each other - the launchers of the operator modes 0 / 1, 5 / 4 / 7 and 2, called by
// the entry unit and defined one per unit.  Included by all four IPCS units, behind the reference tables.
namespace mdq {

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

}  // namespace mdq
