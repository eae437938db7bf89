// IPCS: the last-error state, the descriptor check and the entry points (extern "C" API, ipcs_evolve_impl with the launch
// sequence of mode 3, mdq_probe_forces).  Included by mdq_ipcs.hip (the entry unit) only, at its end.
namespace mdq {

#ifdef MDQ_AT_TRACE
// debug build only: the host halves of the AT / PT / CT stamps (buffers and macros: mdq_ipcs_pressure.hip)
extern "C" MDQ_API int mdq_at_trace_host(long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mdq_at_trace_buf), sizeof(long long) * 16) != hipSuccess) return -1;
  if (reset) { long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(mdq_at_trace_buf), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
extern "C" MDQ_API int mdq_pt_trace_host(long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mdq_pt_trace_buf), sizeof(long long) * 16) != hipSuccess) return -1;
  if (reset) { long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(mdq_pt_trace_buf), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
extern "C" MDQ_API int mdq_ct_trace_host(long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mdq_ct_trace_buf), sizeof(long long) * 16) != hipSuccess) return -1;
  if (reset) { long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(mdq_ct_trace_buf), z, sizeof z) != hipSuccess) return -1; }
  return 0;
}
#endif

static thread_local std::string g_err;

static int fail(const char* what, hipError_t e) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return -1;
}
static int fail_msg(const std::string& m) {
  g_err = m;
  return -2;
}

static int ensure_tables() {
  const hipError_t err = upload_tables();
  if (err != hipSuccess) return fail("hipMemcpyToSymbol(c_tab)", err);
  return 0;
}

// the largest N2 whose vectors fit the LDS of mode 3 (p, r, result) / mode 1 (p, r) behind the reduction scratch - what the
// error texts state; ipcs_batch.operator_mode_limits mirrors these and lds_plan
static int mode3_max_rows() {
  const int lds = (int)((160 * 1024 - 64 * sizeof(double)) / (3 * sizeof(double2))) & ~1;
  return lds < MF_ROWS * WG ? lds : MF_ROWS * WG;
}
static int mode1_max_rows() { return (int)((160 * 1024 - 64 * sizeof(double)) / (2 * sizeof(double2))) & ~1; }

static int check_desc(const mdq_ipcs_desc* d) {
  if (!d) return fail_msg("null descriptor");
  if (d->B <= 0 || d->NV <= 0 || d->NT <= 0 || d->NE <= 0) return fail_msg("bad batch sizes");
  if (d->N2 != d->NV + d->NE) return fail_msg("N2 must equal NV+NE");
  if (d->work_doubles < (int64_t)d->B * work_per_env(d->NV, d->NT, d->NE))
    return fail_msg("workspace too small (see mdq_ipcs_workspace_doubles)");
  if (!(d->dt > 0.0) || !(d->rho > 0.0)) return fail_msg("dt and rho must be positive");
  return 0;
}

}  // namespace mdq

// shared by the other translation units of the library (mdq_internal.h)
int mdq_set_error(const char* msg) {
  mdq::g_err = msg;
  return -2;
}

using namespace mdq;

extern "C" {

int mdq_abi_version(void) { return MDQ_ABI_VERSION; }

const char* mdq_last_error(void) { return g_err.c_str(); }

int64_t mdq_ipcs_workspace_doubles(int32_t B, int32_t NV, int32_t NT, int32_t NE) {
  return (int64_t)B * work_per_env(NV, NT, NE);
}

int mdq_ipcs_reset_history(const mdq_ipcs_desc* d, int32_t* iters, void* stream) {
  if (int rc = check_desc(d)) return rc;
  hipLaunchKernelGGL(reset_history_kernel, dim3((d->B + 63) / 64), dim3(64), 0, (hipStream_t)stream, *d, iters);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail("reset_history_kernel launch", e);
  return 0;
}

int mdq_ipcs_assemble(const mdq_ipcs_desc* d, void* stream) {
  if (int rc = check_desc(d)) return rc;
  if (int rc = ensure_tables()) return rc;
  hipLaunchKernelGGL(assemble_kernel, dim3(d->B), dim3(WG), 0, (hipStream_t)stream, *d);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail("assemble_kernel launch", e);
  return 0;
}

int mdq_ipcs_setup_matfree(const mdq_ipcs_desc* d, void* stream) {
  if (int rc = check_desc(d)) return rc;
  if (!d->coords || !d->cell_dofs || !d->cell_outflow || !d->g1_ptr || !d->g1_src || !d->g2_ptr || !d->g2_src ||
      !d->sl1_off || !d->sl1_col || !d->bcu_flag || !d->bcu_gx || !d->bcp_flag || !d->geom || !d->lift1 || !d->lift3 ||
      !d->idiag1 || !d->sdiagM || !d->sdiagK || !d->K1s)
    return fail_msg("mdq_ipcs_setup_matfree: incomplete descriptor");
  if (d->nbo && (!d->bo_rows || !d->bo_ptr || !d->bo_col || !d->bo_src || !d->bo_val))
    return fail_msg("mdq_ipcs_setup_matfree: outflow row list incomplete");
  if (int rc = ensure_tables()) return rc;
  // staged instance when the mesh's per-cell / per-dof data fit the LDS beside the kernel's static tables
  const size_t stage_bytes = 52 * (size_t)d->NT + 9 * (size_t)d->N2 + 9 * (size_t)d->NV + 64;
  hipError_t e;
  // + the slot lists (16-bit: slot ids < 6 NT <= 65535, pointers likewise) when they fit as well
  const size_t list_bytes = 2 * ((size_t)d->N2 + 1 + 6 * (size_t)d->NT + (size_t)d->NV + 1 + 3 * (size_t)d->NT) + 2;
  if (stage_bytes + list_bytes <= 156 * 1024 && 6 * (size_t)d->NT <= 65535) {
    const size_t bytes = stage_bytes + list_bytes;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&setup_matfree_kernel<true, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail("setup_matfree_kernel attribute", e);
    hipLaunchKernelGGL((setup_matfree_kernel<true, true>), dim3(d->B), dim3(SWG), bytes, (hipStream_t)stream, *d);
  } else if (stage_bytes <= 156 * 1024) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&setup_matfree_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)stage_bytes);
    if (e != hipSuccess) return fail("setup_matfree_kernel attribute", e);
    hipLaunchKernelGGL(setup_matfree_kernel<true>, dim3(d->B), dim3(SWG), stage_bytes, (hipStream_t)stream, *d);
  } else if (const size_t idx_bytes = 12 * (size_t)d->NT + (size_t)d->N2 + 9 * (size_t)d->NV + 64;
             idx_bytes <= 156 * 1024 && d->N2 <= 65535 && std::getenv("MDQ_SETUP_UNSTAGED") == nullptr) {
    // (the index data alone: cell dofs, flags, the P1 scaling; MDQ_SETUP_UNSTAGED=1: the unstaged instance, A / B switch)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&setup_matfree_kernel<true, false, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)idx_bytes);
    if (e != hipSuccess) return fail("setup_matfree_kernel attribute", e);
    hipLaunchKernelGGL((setup_matfree_kernel<true, false, false>), dim3(d->B), dim3(SWG), idx_bytes, (hipStream_t)stream, *d);
  } else {
    hipLaunchKernelGGL(setup_matfree_kernel<false>, dim3(d->B), dim3(SWG), 0, (hipStream_t)stream, *d);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return fail("setup_matfree_kernel launch", e);
  return 0;
}

static int ipcs_evolve_impl(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift, int32_t* iters,
                            const double* inflow_scale, void* stream, double* kernel_ms, int fresh = 0,
                            const mdq_inflow_profile* prof = nullptr);

// the argument checks of the two inflow-profile entry points (`entry`: the name their messages carry), then the step loop
static int evolve_profile_checked(const char* entry, int fresh, const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift,
                                  int32_t* iters, const mdq_inflow_profile* prof, void* stream) {
  if (prof) {
    const auto bad = [entry](const char* what) { return fail_msg(std::string(entry) + what); };
    if (prof->NIN <= 0 || prof->NIR <= 0) return bad(": NIN and NIR must be positive");
    if (!prof->n_inlet || !prof->inlet_dofs || !prof->n_rows || !prof->rows || !prof->values)
      return bad(": incomplete inflow profile (n_inlet, inlet_dofs, n_rows, rows, values)");
    if (d && (!d->cell_dofs || !d->g2_ptr || !d->g2_src || !d->bcu_flag || !d->bcu_gx || !d->geom || !d->lift1 || !d->lift3))
      return bad(": incomplete descriptor (cell_dofs, g2_ptr, g2_src, bcu_flag, bcu_gx, geom, lift1, lift3)");
  }
  return ipcs_evolve_impl(d, nsteps, drag, lift, iters, nullptr, stream, nullptr, fresh, prof);
}

int mdq_ipcs_evolve_profile(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift, int32_t* iters,
                            const mdq_inflow_profile* prof, void* stream) {
  return evolve_profile_checked("mdq_ipcs_evolve_profile", 0, d, nsteps, drag, lift, iters, prof, stream);
}

int mdq_ipcs_evolve_fresh_profile(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift, int32_t* iters,
                                  const mdq_inflow_profile* prof, void* stream) {
  return evolve_profile_checked("mdq_ipcs_evolve_fresh_profile", 1, d, nsteps, drag, lift, iters, prof, stream);
}

int mdq_ipcs_build_inlet_map(const mdq_ipcs_desc* d, int32_t NIN, int32_t NIR, const int32_t* n_ref, const double* inlet_y,
                             int32_t* n_inlet, int32_t* inlet_dofs, int32_t* n_rows, int32_t* rows, int32_t* map_status,
                             void* stream) {
  if (!d || d->B <= 0 || d->NV <= 0 || d->NT <= 0 || d->NE <= 0 || d->N2 != d->NV + d->NE)
    return fail_msg("mdq_ipcs_build_inlet_map: bad batch sizes");
  if (!d->nv || !d->nt || !d->ne || !d->coords || !d->cell_dofs || !d->cell_outflow || !d->bcu_flag || !d->bcu_gx)
    return fail_msg("mdq_ipcs_build_inlet_map: incomplete descriptor (nv, nt, ne, coords, cell_dofs, cell_outflow, bcu_flag, bcu_gx)");
  if (d->N2 > MAP_BITS)
    return fail_msg("mdq_ipcs_build_inlet_map: N2 > " + std::to_string(MAP_BITS) + " (the inlet map serves the meshes of operator mode 3)");
  if (NIN <= 0 || NIN > MAP_NIN || NIR <= 0)
    return fail_msg("mdq_ipcs_build_inlet_map: NIN must be in 1 .. " + std::to_string(MAP_NIN) + " and NIR positive");
  if (!n_ref || !inlet_y || !n_inlet || !inlet_dofs || !n_rows || !rows || !map_status)
    return fail_msg("mdq_ipcs_build_inlet_map: null table (n_ref, inlet_y, n_inlet, inlet_dofs, n_rows, rows, map_status)");
  hipLaunchKernelGGL(inlet_map_kernel, dim3(d->B), dim3(MWG), 0, (hipStream_t)stream, *d, NIN, NIR, n_ref, inlet_y, n_inlet,
                     inlet_dofs, n_rows, rows, map_status);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail("inlet_map_kernel launch", e);
  return 0;
}

int mdq_ipcs_evolve(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift, int32_t* iters,
                    void* stream) {
  return ipcs_evolve_impl(d, nsteps, drag, lift, iters, nullptr, stream, nullptr);
}

int mdq_ipcs_evolve_inflow(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift, int32_t* iters,
                           const double* inflow_scale, void* stream) {
  return ipcs_evolve_impl(d, nsteps, drag, lift, iters, inflow_scale, stream, nullptr);
}

int mdq_ipcs_evolve_fresh(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift, int32_t* iters,
                          const double* inflow_scale, void* stream) {
  return ipcs_evolve_impl(d, nsteps, drag, lift, iters, inflow_scale, stream, nullptr, 1);
}

int mdq_ipcs_evolve_timed(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift, int32_t* iters,
                          void* stream, double* kernel_ms) {
  if (!kernel_ms) return fail_msg("kernel_ms is required");
  if (d && d->mode != 3 && d->mode != -1) return fail_msg("per-kernel timing exists for the three-kernel mode 3 only");
  return ipcs_evolve_impl(d, nsteps, drag, lift, iters, nullptr, stream, kernel_ms);
}

static int ipcs_evolve_impl(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift, int32_t* iters,
                            const double* inflow_scale, void* stream, double* kernel_ms, int fresh,
                            const mdq_inflow_profile* prof) {
  if (int rc = check_desc(d)) return rc;
  if (nsteps <= 0) return fail_msg("nsteps must be positive");
  if (!drag || !lift) return fail_msg("drag/lift output pointers are required");
  if (int rc = ensure_tables()) return rc;
  const LdsPlan P = lds_plan(d->N2, d->NV, d->NSE1);
  const size_t LDS_MAX = 160 * 1024, red_bytes = 64 * sizeof(double);
  // pressure CG vectors beyond the LDS: kept in the workspace slab (modes 0 / 5; Jacobi-CG only - the factorisation has
  // its own, smaller limits and reports such a mesh through pd_status)
  const bool pg = red_bytes + P.prs_vec_bytes > LDS_MAX;
  // (pd_enabled with pg: the factors' own limits are far below this size - every such environment has nparts = 0 and
  //  takes the Krylov branch anyway; a small mesh riding along in the big layout is solved by CG as well)
  const bool k1_lds = !pg && !d->pd_enabled && red_bytes + P.prs_vec_bytes + P.prs_mat_bytes <= LDS_MAX;
  int mode = d->mode;
  // mode 5: the element tile (+ the stage of a chunk's input rows behind it when the packed local maps are given and fit)
  const size_t tile_bytes = tile_lds_bytes(*d);
  if (mode == 6) return fail_msg("unknown operator mode 6");
  // what the descriptor carries: a mode is chosen (auto) or accepted (explicit) only with the arrays its kernels read - a
  // matrix-free descriptor (flow leg, device-built index data) has no assembled operators and no tile pointers
  const bool has_asm = d->A1 && d->Ms && d->sl2_off && d->sl2_col;                      // modes 0 / 1 / 4
  const bool has_mf = d->mf_scat && d->mf_tptr;                                         // mode 2 (packed words + tile pointers)
  const bool has_tiles = d->cell_outflow && (has_mf || (d->g2_ptr && d->g2_src));       // modes 5 / 7
  const bool fits1 = red_bytes + P.vel1_bytes <= LDS_MAX;
  const bool fits2 = red_bytes + P.vel2_bytes <= LDS_MAX && d->N2 <= MF_ROWS * WG;
  const bool fits3 = red_bytes + P.vel3_bytes <= LDS_MAX && d->N2 <= MF_ROWS * WG;
  if (mode < 0 || mode > 7) {  // auto: fastest variant that fits
    mode = 0;
    if (has_asm && fits1) mode = 1;
    if (has_mf && fits2) mode = 2;
    // (mode -2 = auto among the BITWISE REPRODUCIBLE variants: everything but the LDS-atomic mode 3)
    if (d->mode != -2 && d->mf_scat && fits3) mode = 3;
    // a mesh beyond the LDS-resident vectors, or a descriptor without the arrays of the modes above: the element tiles with
    // global vectors (mode 5: ~5x less memory traffic than the assembled operators and no sparsity pattern), when the tile
    // maps or the slot lists were handed over
    if (mode == 0 && has_tiles && std::getenv("MDQ_NO_MODE5") == nullptr) mode = 5;
    if (mode == 0 && !has_asm)
      return fail_msg("no operator mode fits this descriptor: the assembled operators (A1, Ms, sl2_off, sl2_col) are missing and so "
                      "are cell_outflow with the tile maps (mf_scat, mf_tptr) or the dof <- slot lists (g2_ptr, g2_src)");
    if (mode == 0) {
      // a mesh that only fits the assembled global-memory path: two workgroups per environment while the batch leaves
      // at least half of the chip idle even so (measured on ys930 red-refined, ms per step one / two workgroups: B = 1
      // 13.7 / 8.0, 32: 16.7 / 11.9, 64: 24.5 / 22.0, 96: 26.0 / 29.3, 128: 20.0 / 26.1 - from ~64 environments on the
      // step is bound by the memory system as a whole, and the team barriers' cache write-backs / invalidations only add)
      const int ncu = team_cus((hipStream_t)stream);
      if (!pg && 2 * TEAM * d->B <= ncu) mode = 4;
    }
    // the element tiles with TWO workgroups per environment while the batch leaves half of the chip idle (BASELINE batch of
    // 128 refined meshes: 11.3 -> ms per step; MDQ_NO_TEAM_TILES=1 is the A / B switch)
    if (mode == 5 && !pg && std::getenv("MDQ_NO_TEAM_TILES") == nullptr) {
      if (TEAM * d->B <= team_cus((hipStream_t)stream)) mode = 7;
    }
  }
  if (kernel_ms && mode != 3) return fail_msg("per-kernel timing exists for the three-kernel mode 3 only");
  // an inflow profile is rewritten BETWEEN the steps of a launch sequence: the modes that loop over the steps inside one kernel
  // have no such place
  if (prof && mode != 2 && mode != 3)
    return fail_msg("mdq_ipcs_evolve_profile: operator mode " + std::to_string(mode) + " runs the steps of a call inside one kernel; "
                    "an inflow profile is served by the per-step path (operator modes 2 and 3, or mdq_ipcs_setup_matfree + "
                    "mdq_ipcs_evolve one step at a time)");
  // every refusal comes before the first launch
  if (mode == 3 && !fits3)
    return fail_msg("mode 3 needs N2 <= " + std::to_string(mode3_max_rows()) + " (three velocity vectors of N2 rows in " +
                    std::to_string(LDS_MAX / 1024) + " KB of LDS, at most " + std::to_string(MF_ROWS * WG) + " rows)");
  if (mode == 3 && !d->mf_scat) return fail_msg("mode 3 needs the packed element words (mf_scat)");
  if (mode == 2 && !fits2)
    return fail_msg("matrix-free tile mode needs N2 <= " + std::to_string(MF_ROWS * WG) + " and the x stage + element tile in LDS");
  if (mode == 2 && !has_mf) return fail_msg("mode 2 needs the packed element words and the tile pointers (mf_scat, mf_tptr)");
  if (mode == 1 && !fits1)
    return fail_msg("LDS gather vectors do not fit (mode 1 needs N2 <= " + std::to_string(mode1_max_rows()) + ")");
  if ((mode == 0 || mode == 1 || mode == 4) && !has_asm)
    return fail_msg("modes 0 / 1 / 4 need the assembled operators (A1, Ms, sl2_off, sl2_col): this descriptor is matrix-free only "
                    "(use mode -1, 5 or 7)");
  if ((mode == 5 || mode == 7) && !has_tiles)
    return fail_msg("modes 5 / 7 need cell_outflow and the tile maps (mf_scat, mf_tptr) or the dof <- slot lists (g2_ptr, g2_src)");
  if (pg && mode != 0 && mode != 5)
    return fail_msg("mesh too large for the LDS-resident pressure vectors of this operator mode (use mode -1, 0 or 5)");
  // a fresh history: mode 3 drops it inside the kernels of its first step; the one-kernel modes take the reset launch
  if (fresh && mode != 3) {
    hipLaunchKernelGGL(reset_history_kernel, dim3((d->B + 63) / 64), dim3(64), 0, (hipStream_t)stream, *d, iters);
    if (hipError_t e_ = hipGetLastError(); e_ != hipSuccess) return fail("reset_history_kernel launch", e_);
  }
  // (K1 values alias the scratch vector: CG does not use it; pg: the tables of the two-level preconditioner)
  size_t u = pg ? tl_extra_bytes(d->NV) + sizeof(double) * NAG * NAG : P.prs_vec_bytes + (k1_lds ? P.prs_mat_bytes : 0);
  const size_t vel = mode == 3 ? P.vel3_bytes : (mode == 2 ? P.vel2_bytes : (mode == 1 ? P.vel1_bytes : ((mode == 5 || mode == 7) ? tile_bytes : 0)));
  if (vel > u) u = vel;
  const size_t lds = red_bytes + u;
  hipError_t e;
  hipStream_t st = (hipStream_t)stream;
  if (mode == 3) {
    const size_t lds_v = red_bytes + P.vel3_bytes;
    const size_t lds_p = red_bytes + P.prs_vec_bytes + (k1_lds ? P.prs_mat_bytes : 0);
    const size_t lds_c = red_bytes + 2 * sizeof(double2) * (size_t)P.N2p + sizeof(double) * (size_t)P.NVp;  // p, result, dp
    // once per process (thread-safe: several env groups call this entry point concurrently)
    static const hipError_t attr_err = [] {
      hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&at_velocity_kernel<WG, MF_ROWS, AT_PAIR>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e_ == hipSuccess)
        e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&at_velocity_kernel<768, 5, 1>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e_ == hipSuccess)
        e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&at_pressure_kernel<true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e_ == hipSuccess)
        e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&at_pressure_kernel<false>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e_ == hipSuccess)
        e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&at_pressure_kernel<false, 1024>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e_ == hipSuccess)
        e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&at_correction_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      return e_;
    }();
    if (attr_err != hipSuccess) return fail("hipFuncSetAttribute(mode 3 kernels)", attr_err);
    // velocity kernel variant: 12 waves x 1 triangle stream (3 waves per SIMD, <= 170 VGPRs) or 8 waves x 2 interleaved
    // triangle streams (2 per SIMD, 256 VGPRs); MDQ_AT_WG=512|768 overrides
    static const int vel_wg = [] {
      const char* s_ = std::getenv("MDQ_AT_WG");
      const int w_ = s_ ? std::atoi(s_) : 768;
      return w_ == 512 ? 512 : 768;
    }();
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (kernel_ms) {
      for (int i = 0; i < 4; ++i)
        if ((e = hipEventCreate(&ev[i])) != hipSuccess) return fail("hipEventCreate", e);
      kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
    }
    for (int step = 0; step < nsteps; ++step) {
      if (prof)
        if ((e = launch_inflow_lift(d, prof, nsteps, step, st)) != hipSuccess) return fail("inflow_lift_kernel launch", e);
      if (kernel_ms) hipEventRecord(ev[0], st);
      if (vel_wg == 768)
        hipLaunchKernelGGL((at_velocity_kernel<768, 5, 1>), dim3(d->B), dim3(768), lds_v, st, *d, iters, inflow_scale, nsteps, step, fresh);
      else
        hipLaunchKernelGGL((at_velocity_kernel<WG, MF_ROWS, AT_PAIR>), dim3(d->B), dim3(WG), lds_v, st, *d, iters, inflow_scale, nsteps, step, fresh);
      if (kernel_ms) hipEventRecord(ev[1], st);
      if (d->pd_enabled)
        hipLaunchKernelGGL((at_pressure_kernel<false, 1024>), dim3(d->B), dim3(1024), lds_p, st, *d, iters, fresh && step == 0);
      else if (k1_lds)
        hipLaunchKernelGGL(at_pressure_kernel<true>, dim3(d->B), dim3(WG), lds_p, st, *d, iters, fresh && step == 0);
      else
        hipLaunchKernelGGL(at_pressure_kernel<false>, dim3(d->B), dim3(WG), lds_p, st, *d, iters, fresh && step == 0);
      if (kernel_ms) hipEventRecord(ev[2], st);
      hipLaunchKernelGGL(at_correction_kernel, dim3(d->B), dim3(WG), lds_c, st, *d, nsteps, step, drag, lift, iters, inflow_scale, fresh);
      if (kernel_ms) {
        hipEventRecord(ev[3], st);
        if ((e = hipEventSynchronize(ev[3])) != hipSuccess) return fail("hipEventSynchronize", e);
        for (int i = 0; i < 3; ++i) {
          float ms = 0.f;
          hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
          kernel_ms[i] += ms;
        }
      }
    }
    if (kernel_ms)
      for (int i = 0; i < 4; ++i) hipEventDestroy(ev[i]);
    e = hipGetLastError();
  } else {
    const EvolveArgs a{d, lds, nsteps, drag, lift, iters, inflow_scale, st, prof};
    if (mode == 2)
      e = part_launch_mf(k1_lds, a);
    else if (mode == 4 || mode == 5 || mode == 7)
      e = part_launch_tiles(mode, k1_lds, pg, a);
    else
      e = part_launch_assembled(mode, k1_lds, pg, a);
  }
  if (e != hipSuccess) return fail("evolve_kernel launch", e);
  return 0;
}

int mdq_probe_forces(const mdq_ipcs_desc* d, int32_t nfields, const double* u, const double* p, double* drag,
                     double* lift, void* stream) {
  // needs only: B, NV, NT, NE, N2, NAF, mu, nv, nt, ne, naf, coords, cell_dofs, af_facets
  if (!d || d->B <= 0 || d->N2 != d->NV + d->NE || !d->coords || !d->cell_dofs || !d->af_facets)
    return fail_msg("mdq_probe_forces: incomplete mesh descriptor");
  if (nfields <= 0 || !u || !p || !drag || !lift) return fail_msg("bad probe arguments");
  if (int rc = ensure_tables()) return rc;
  hipLaunchKernelGGL(probe_kernel, dim3(d->B), dim3(WG), 0, (hipStream_t)stream, *d, nfields, u, p, drag, lift);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail("probe_kernel launch", e);
  return 0;
}

}  // extern "C"
