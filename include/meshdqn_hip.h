/*
 * meshdqn_hip.h - C ABI of the MI355X (gfx950) hot path of MeshDQN.
 *
 * Drop-in boundary for the data-parallel hot path of BaratiLab/MeshDQN
 * (Env2DAirfoil rollout = Taylor-Hood IPCS Navier-Stokes solve + graph
 * Q-network forward).  The reference has no native code and no FFI: all of its
 * arithmetic sits behind Python calls into DOLFIN / PyG.  Each entry point
 * below names the reference call site (file:line in BaratiLab/MeshDQN) whose
 * arithmetic it replaces; the Python classes in `meshdqn_amd/` that keep the
 * reference's `FlowSolver` / `Env2DAirfoil` / `NodeRemovalNet` surfaces bind
 * these symbols through ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch types.
 *   - every call returns int: 0 = ok, <0 = error (text via mdq_last_error()).
 *   - all array arguments marked "device" are DEVICE pointers borrowed from
 *     the caller (torch tensors); the library never frees them and performs no
 *     hidden allocation; work is enqueued on the given hipStream_t (passed as
 *     void*; NULL = default stream) and the call returns without a device sync.
 *     Scratch memory is ALWAYS the caller's: every entry point that needs some
 *     takes a `workspace` (+ its size in bytes) whose minimum size a
 *     `*_workspace_bytes` / `*_workspace_doubles` query returns (0: none needed;
 *     < 0: the sizes are beyond the kernels); launches that may overlap - other
 *     streams - need workspaces of their own.  (ABI 5 kept the tables of the
 *     large-mesh kernel instances in process-static slabs grown with hipMalloc
 *     inside the calls: that broke this rule and is gone.)
 *   - "host" arguments are ordinary host pointers.
 *   - not re-entrant per batch descriptor; independent descriptors may be used
 *     from independent streams / processes.
 *
 * Batch layout: B environments, every per-environment array padded to common
 * capacities (NV vertices, NT triangles, NE edges, N2 = NV+NE scalar P2 dofs,
 * NNZ2 / NNZ1 non-zeros of the P2 / P1 CSR patterns, NSE2 / NSE1 entries of
 * their SELL-64 layouts); actual sizes in the
 * per-environment count arrays.  Velocity vectors are component-interleaved:
 * u[dof][c], dof in [0,N2), c in {x,y}.
 */
#ifndef MESHDQN_HIP_H
#define MESHDQN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDQ_ABI_VERSION 8

/* The library is built with -fvisibility=hidden: the entry points below are its ONLY exported symbols. */
#if defined(__GNUC__)
#define MDQ_API __attribute__((visibility("default")))
#else
#define MDQ_API
#endif

/* ---- error handling ----------------------------------------------------- */
MDQ_API int mdq_abi_version(void);
MDQ_API const char* mdq_last_error(void);

/* ---- IPCS batch descriptor ---------------------------------------------- */
typedef struct mdq_ipcs_desc {
  /* sizes */
  int32_t B;            /* environments in the batch                         */
  int32_t NV, NT, NE;   /* per-environment capacities                        */
  int32_t N2;           /* NV + NE (scalar P2 dof capacity)                  */
  int32_t NNZ2, NNZ1;   /* CSR capacities of the P2 / P1 patterns            */
  int32_t NAF;          /* capacity of the airfoil (tag 1) facet list        */
  int32_t NSE2, NSE1;   /* SELL-64 entry capacities of the P2 / P1 operators */
  /* physics: flow_params / solver_params of FlowSolver (flow_solver.py:49-52,95); batch-wide unless env_phys (the
     struct's last field) is set */
  double mu, rho, dt;
  /* Krylov controls (the reference uses MUMPS LU, flow_solver.py:150-151;
     these bound the error of the iterative replacement) */
  double rtol;          /* relative residual tolerance (preconditioned norm) */
  int32_t maxit_u, maxit_p, maxit_m;
  int32_t mode;         /* operator application: -1 auto (fastest that fits), -2 auto among the BITWISE REPRODUCIBLE
                           variants (everything but 3: what ground truths / re-simulations of thousands of steps run
                           on, deploy_dqn.py:262-269, Env2DAirfoil.py:111-125), 0 assembled SELL (global gather vectors),
                           1 assembled SELL (LDS gather vectors), 2 matrix-free LDS element tiles (bitwise
                           reproducible), 3 matrix-free with LDS fp64 atomics (fastest; round-off reproducible),
                           4 assembled SELL with TWO workgroups per environment (any mesh size, rows / cells / slices
                           dealt out over the team, agent-scope team barriers; auto picks it over 0 when 4 B <= CUs),
                           5 matrix-free element tiles with the vectors in GLOBAL memory (any mesh size: what auto takes for
                           meshes beyond the LDS-resident vectors of 2 / 3 when mf_scat / mf_tptr are given; bitwise reproducible),
                           7 the element tiles of 5 with TWO workgroups per environment (chunks dealt out alternately, one
                           accumulation vector per workgroup; bitwise reproducible run to run, a row's sum associated
                           differently from 5; what auto takes instead of 5 while 2 B <= CUs).  6 is not a mode.
                           Size limits (160 KB of LDS): 1 up to N2 = 5104, 2 up to 3584, 3 up to 3402 (three vectors).  A mode
                           is chosen (auto) or accepted (explicit) only when the descriptor carries the arrays its kernels
                           read - 0 / 1 / 4: A1, Ms, sl2_off, sl2_col; 2: mf_scat + mf_tptr; 3: mf_scat; 5 / 7: cell_outflow
                           with mf_scat + mf_tptr or g2_ptr + g2_src - and every refusal comes before the first launch: a
                           matrix-free descriptor (no assembled operators) beyond mode 3 runs the element tiles. */
  /* per-environment counts, device int32[B] */
  const int32_t* nv;
  const int32_t* nt;
  const int32_t* ne;
  const int32_t* naf;
  /* mesh, device */
  const double* coords;        /* [B][NV][2]  (smoothed) vertex coordinates   */
  const int32_t* cell_dofs;    /* [B][6][NT]  P2 dofs per cell: 3 vertices (ascending), 3 edge dofs NVenv+edge */
  const int8_t* cell_outflow;  /* [B][NT]     local edge (0..2) lying on the outflow boundary, or -1 */
  /* CSR patterns + deterministic gather maps, device */
  const int32_t* rowptr2;      /* [B][N2+1]   */
  const int32_t* colidx2;      /* [B][NNZ2]   */
  const int32_t* asm2_ptr;     /* [B][NNZ2+1] non-zero <- element slots       */
  const int32_t* asm2_src;     /* [B][36*NT]  slot = cell*36 + i*6 + j        */
  const int32_t* rowptr1;      /* [B][NV+1]   */
  const int32_t* colidx1;      /* [B][NNZ1]   */
  const int32_t* asm1_ptr;     /* [B][NNZ1+1] */
  const int32_t* asm1_src;     /* [B][9*NT]   slot = cell*9 + i*3 + j         */
  /* SELL-64 layout of the same patterns (slices of 64 consecutive rows, column-major
     inside a slice, width = longest row of the slice, padding column = own row) */
  const int32_t* sl2_off;      /* [B][N2/64+2]  slice offsets in entries      */
  const int32_t* sl2_col;      /* [B][NSE2]   */
  const int32_t* sl1_off;      /* [B][NV/64+2] */
  const int32_t* sl1_col;      /* [B][NSE1]   */
  /* matrix-free tile maps (mode 2): chunks of 1024 consecutive triangles          */
  const int32_t* mf_scat;      /* [B][6][NT]  packed: dof | tile position << 12 | (outflow edge + 1) << 28 (word 0); tile entries ordered by (row, triangle) */
  const int32_t* mf_tptr;      /* [B][NCH][N2+1] row r owns tile entries [tptr[r], tptr[r+1]) of chunk c; NCH = (NT+1023)/1024 */
  const int32_t* g2_ptr;       /* [B][N2+1]   P2 dof <- element slots         */
  const int32_t* g2_src;       /* [B][6*NT]   slot = cell*6 + i               */
  const int32_t* g1_ptr;       /* [B][NV+1]   */
  const int32_t* g1_src;       /* [B][3*NT]   slot = cell*3 + i               */
  /* Dirichlet data (flow_solver.py:123-132), device */
  const uint8_t* bcu_flag;     /* [B][N2]  1 = velocity dof constrained (both components) */
  const double* bcu_gx;        /* [B][N2]  x-velocity value (y value is 0)    */
  const uint8_t* bcp_flag;     /* [B][NV]  1 = pressure dof constrained to 0  */
  /* outflow-facet term of F1 (`- dot(mu*nabla_grad(U)*n, v)*ds`, flow_solver.py:109) as a tiny row list
     for the matrix-free mode 3: row r owns entries [bo_ptr[t], bo_ptr[t+1]) with 2x2 blocks
     B^{cd} = int_facet phi_r (d_c phi_col) n_d ds; values written by mdq_ipcs_assemble */
  int32_t NBO, NBE;            /* capacities: outflow rows, entries                 */
  const int32_t* nbo;          /* device [B]  number of outflow rows                */
  const int32_t* bo_rows;      /* device [B][NBO]   P2 dof of the row               */
  const int32_t* bo_ptr;       /* device [B][NBO+1]                                 */
  const int32_t* bo_col;       /* device [B][NBE]   P2 dof of the column            */
  const int32_t* bo_src;       /* device [B][NBE]   cell*36 + i*6 + j (local test / trial index) */
  double* bo_val;              /* device [B][NBE][4] (out) xx, xy, yx, yy           */
  /* direct (substructured) pressure solver, written by the host after assembly
     (meshdqn_amd/pressure_direct.py; replaces the reference's MUMPS factorisation of A2,
     flow_solver.py:150-159).  pd_enabled = 0 -> Jacobi-CG on the SELL operator instead. */
  int32_t pd_enabled;
  int32_t NPART, NPW, NPF, NPGI, NPS, NPGK;   /* capacities of the arrays below */
  int32_t pcg_degree;          /* mode 3, Krylov pressure solve (pd_enabled = 0 or no factors): degree m of the Chebyshev
                                  polynomial preconditioner of the CG on the Jacobi-scaled P1 Laplacian (m - 1 extra
                                  operator applications per iteration, no extra reductions); 0 / 1 = Jacobi only;
                                  < 0 = two-level additive preconditioner (8 x 7 geometric aggregates, coarse matrix
                                  inverted in LDS): fewer operator applications (167 -> ~100 iterations on ys930).
                                  Modes 0 / 4 / 5 / 7 (the meshes beyond mode 3; pressure vectors in LDS or, beyond
                                  ~4 000 vertices, in the workspace): 0 = auto - Jacobi-CG below 2048 vertices, the two-level
                                  preconditioner with an O(n) aggregation from there (refined ys930, 3 322 vertices: 325 ->
                                  158 iterations; refined twice, 12 924 vertices: 833 -> 470) -, < 0 = two-level wherever its
                                  scratch fits, > 0 = Jacobi-CG */
  const int32_t* pd_hdr;       /* [B][4]  nI, nG, nparts, 0                       */
  const int32_t* pd_node;      /* [B][NV] node id of permuted position (interiors by subdomain, then separator) */
  const int32_t* pd_meta;      /* [B][NPART][6] q0, m, W offset, F offset, g, gidx offset */
  const int32_t* pd_rowblk;    /* [B][NV] subdomain of permuted interior row       */
  const double* pd_W;          /* [B][NPW]  inv(K[I_s,I_s]) column-major blocks    */
  const double* pd_F;          /* [B][NPF]  W_s K[I_s,G_s] column-major blocks     */
  const int32_t* pd_gidx;      /* [B][NPGI] separator-local column ids of F blocks */
  const double* pd_Sinv;       /* [B][NPS]  inverse Schur complement, column-major nG x nG */
  const int32_t* pd_gk_ptr;    /* [B][NV+1] CSR of K[G,I] in permuted interior numbering */
  const int32_t* pd_gk_col;    /* [B][NPGK] */
  const double* pd_gk_val;     /* [B][NPGK] */
  /* airfoil facets for the probes (probes.py:23-50), device */
  const int32_t* af_facets;    /* [B][NAF][2] (cell, local edge)              */
  /* assembled operators, device, written by mdq_ipcs_assemble */
  double* geom;                /* [B][5][NT]  Jinv00,Jinv01,Jinv10,Jinv11,|det| */
  double* A1;                  /* [B][NSE2][4] SELL, row-scaled velocity blocks xx,xy,yx,yy */
  double* Ms;                  /* [B][NSE2]   SELL, symmetrically scaled P2 mass (with BCs) */
  double* K1s;                 /* [B][NSE1]   SELL, symmetrically scaled P1 stiffness (with BCs) */
  double* lift1;               /* [B][N2][2]  A1_full[:,bc] g                 */
  double* lift3;               /* [B][N2][2]  M_full[:,bc] g                  */
  double* idiag1;              /* [B][N2][2]  1/diag(A1)                      */
  double* sdiagM;              /* [B][N2]     sqrt(diag(M_bc))                */
  double* sdiagK;              /* [B][NV]     sqrt(diag(K1_bc))               */
  /* state, device */
  double* u_n;                 /* [B][N2][2]  */
  double* p_n;                 /* [B][NV]     */
  /* workspace, device: at least mdq_ipcs_workspace_doubles() doubles */
  double* work;
  int64_t work_doubles;
  /* mode 5 (optional; NULL: the row owners walk mf_tptr): per chunk the rows its 1024 triangles touch, ascending - entry =
     (row, first tile position | number of tile entries << 16) - so that a row phase visits ~2 500 touched rows instead of
     all N2 (12 924 on the refined ys930) */
  const int32_t* mf_rlist;     /* [B][NCH][NRL][2] */
  const int32_t* mf_rcnt;      /* [B][NCH] touched rows of the chunk */
  const int32_t* mf_lpos;      /* [B][6][NT] optional (NULL: off), with mf_rlist: position of dof i of triangle e in its chunk's row
                                  list (bits 0-15) | tile position (bits 16-31, = the plain mf_scat value): the chunk's input rows
                                  are then staged in LDS through the row list instead of gathered per triangle from global memory
                                  (needs NRL rows of 16 bytes behind the 96 KB tile: NRL <= ~3900) */
  int32_t NRL, rl_flags;             /* rl_flags = 1: bit 31 / bit 30 of a list entry's row word mark the FIRST / LAST chunk that
                                        touches the row, and every row < n2 is touched by some chunk (ABI 5, round 4) */
  /* ABI 7 (round 6), optional (NULL: off): [B] STICKY status words of the environments, OR-ed into by mdq_ipcs_evolve and never
     cleared by the library (the caller zeroes them).  MDQ_IPCS_TEAM_TIMEOUT: an IPCS step of the two-workgroup operator modes
     (4 / 7) was abandoned because a team barrier timed out - the partner workgroup was not resident (another process or stream
     held its CU).  That step and the later steps of the launch report NaN drag / lift; u_n / p_n keep the last completed step. */
  int32_t* status;
  /* optional, appended within ABI 8 (NULL: off): per-environment flow constants, device [B][4]; row b = mu, rho, dt, 0 of
     environment b (rows are 32 bytes: the base must be 32-byte aligned).  Set, the kernels of mdq_ipcs_assemble /
     _setup_matfree / _evolve / mdq_probe_forces read the constants of environment b from its row instead of the scalars
     mu / rho / dt above - one batch then spans several Reynolds numbers or time steps.  The scalars are still validated
     (dt, rho > 0): a caller that sets env_phys fills them from row 0.  The entry points cannot read a device table:
     checking that every row is finite and > 0 is the CALLER's job (meshdqn_amd.ipcs_batch.flow_table does it).
     MDQ_ABI_VERSION stays 8: the field is the struct's last one and NULL means what ABI 8 meant, so a caller that
     zero-initialises the descriptor (every ABI 8 caller must: the optional fields above are NULL-is-off as well) and is
     rebuilt against this header behaves as before; no entry point or exported symbol is added. */
  const double* env_phys;
} mdq_ipcs_desc;
#define MDQ_IPCS_TEAM_TIMEOUT 1

/* doubles of workspace needed for a descriptor with the given capacities */
MDQ_API int64_t mdq_ipcs_workspace_doubles(int32_t B, int32_t NV, int32_t NT, int32_t NE);

/*
 * Assemble the three IPCS operators for every environment of the batch.
 * Replaces `SystemAssembler(a1,L1,bcu).assemble(A)` x3 and the UFL forms
 * (flow_solver.py:98-144; same for remesh in DEPLOY mode, :268-316):
 * per-triangle geometry + P2/P1 element matrices -> CSR values by a
 * deterministic gather, symmetric Dirichlet elimination, Jacobi scaling.
 */
MDQ_API int mdq_ipcs_assemble(const mdq_ipcs_desc* d, void* stream);

/*
 * A new mesh in the same descriptor (FlowSolver.remesh, flow_solver.py:233-359: the solvers restart without history): the
 * counters of the extrapolated initial guesses inside the workspace back to zero (the vectors behind them are not read
 * while their counter is zero), and - when `iters` is not NULL - the [B][3] iteration counters too.  Replaces a fill of
 * the whole workspace in front of mdq_ipcs_setup_matfree.
 */
MDQ_API int mdq_ipcs_reset_history(const mdq_ipcs_desc* d, int32_t* iters, void* stream);

/*
 * Operator setup of the MATRIX-FREE path only (mode 3, CG pressure solver) - what `FlowSolver.remesh` would have to
 * redo after every vertex removal (flow_solver.py:268-339 runs it in DEPLOY mode only): per-triangle geometry, the
 * outflow-row blocks, Jacobi diagonals and Dirichlet lifting vectors of A1 / M accumulated row-wise from the element
 * matrices (no global pattern), the scaled P1 Laplacian in SELL-64.  Needs from the descriptor: sizes, coords,
 * cell_dofs, cell_outflow, g1_*, g2_*, sl1_off/sl1_col, bcu_*, bcp_flag, bo_* ; writes geom, bo_val, lift1, lift3,
 * idiag1, sdiagM, sdiagK, K1s.  The pattern pointers (rowptr*, colidx*, asm*, sl2*) and A1/Ms may be NULL; such a
 * descriptor is valid for mdq_ipcs_evolve with mode = 3 and pd_enabled = 0 only.
 */
MDQ_API int mdq_ipcs_setup_matfree(const mdq_ipcs_desc* d, void* stream);

/*
 * ABI 7 (round 6).  The tile maps of the element-tile operator modes (5 / 7) for meshes that exist only on the device - the
 * coarsened meshes of the S3 env step, i.e. what `FlowSolver.remesh` (flow_solver.py:233-359) would derive after every
 * `Env2DAirfoil._remove_vertex` - built from the dof <- element-slot lists mdq_env_topology emits (g2_ptr, g2_src; needs nv, nt,
 * ne as well).  WRITES the arrays the descriptor's mf_rlist [B][NCH][NRL][2], mf_rcnt [B][NCH] and mf_lpos [B][6][NT] point at
 * (device, caller-owned; NCH = ceil(NT / 1024); NRL = row capacity of a chunk's list, <= 4064 for the LDS stage of the kernels):
 * bit for bit what `IpcsBatch` builds on the host for the same cells and dof numbering, with the first / last chunk bits of
 * rl_flags = 1.  mf_scat / mf_tptr stay NULL: mdq_ipcs_evolve takes the row lists + packed local maps alone.  An environment
 * whose maps cannot be built (a chunk that touches more than NRL rows, a dof without a cell) gets mf_rcnt[b][0] = -1 and keeps
 * the path through the element scratch and the dof <- slot lists; `status` (optional, device int32 [B]): 0 / 1 per environment.
 * Limits: NT <= 8192, N2 <= 16384, tables (NCH + 4) * N2 bytes <= 160 KB of LDS.
 */
MDQ_API int mdq_ipcs_build_tile_maps(const mdq_ipcs_desc* d, int32_t* status, void* stream);

/*
 * ABI 7 (round 6).  Spatial order for the cells of a PRIVATE copy of B meshes (the flow engine's input set of the S3 step, in
 * front of mdq_env_topology + mdq_ipcs_build_tile_maps): the cells of every mesh are sorted along a Morton curve of their
 * centroids (ties by cell id: the order is a function of the mesh alone) and `cells` [B][NT][3] and - when not NULL - `cell_dofs`
 * [B][6][NT] (another engine's dofs of the same cells) are permuted alike, in place.  Chunks of 1 024 consecutive triangles then
 * share their rows (~2 500 touched rows per chunk instead of ~5 000 in the order refinement and cavity re-triangulations leave):
 * what the tile maps need.  The reference has no counterpart: DOLFIN's assembly order is the mesh file's cell order
 * (flow_solver.py:123-144) and only the summation order of the element loops depends on it.  NT <= 8192.
 */
MDQ_API int mdq_flow_sort_cells(int32_t B, int32_t NV, int32_t NT, const double* coords, const int32_t* nv, const int32_t* nt,
                                int32_t* cells, int32_t* cell_dofs, void* stream);

/*
 * Advance every environment by `nsteps` IPCS time steps.
 * Replaces `FlowSolver.evolve()` (flow_solver.py:362-396): per step three
 * right-hand-side assemblies, three linear solves (BiCGStab / CG / CG in place
 * of the MUMPS back-substitutions), u_n/p_n update and the drag / lift probes
 * (probes.py:23-50).
 *   drag, lift : device double[B][nsteps]   (accumulated_drag / accumulated_lift)
 *   iters      : device int32[B][3] or NULL; Krylov iterations of the three
 *                solves are ADDED to it (velocity, pressure, correction)
 * State carried between calls: u_n, p_n and (mode 3) the tentative-velocity history in `work` from which the initial
 * guess of the velocity solve is extrapolated.  Zero `work` whenever u_n / p_n are replaced from outside or the mesh
 * changes (stale history only costs iterations, never accuracy: every solve still runs to `rtol`).
 */
MDQ_API int mdq_ipcs_evolve(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift,
                    int32_t* iters, void* stream);

/*
 * mdq_ipcs_evolve under a per-environment, time-dependent SEPARABLE inflow u_x(inlet, t) = a_b(t) * parabola(y)
 * (the reference's `inflow_profile` evaluated per step, flow_solver.py:366-371, for profiles of that form).
 *   inflow_scale : device double[B][nsteps], laid out like drag / lift: entry [b][s] is the factor a_b that step s of THIS
 *                  launch applies to environment b's inlet values.  NULL: exactly mdq_ipcs_evolve.
 * Every velocity boundary condition but the inlet is zero and the symmetric elimination is linear in the Dirichlet vector,
 * so g(t) = a g0, lift1(t) = a lift1_0, lift3(t) = a lift3_0 and the pressure lifting is zero: the kernels multiply every
 * read of bcu_gx / lift1 / lift3 by the step's factor and rewrite nothing - the descriptor (set up ONCE, for a = 1) serves
 * any schedule.  A table of ones gives the bits of NULL in the fixed-order modes.
 * The entry point cannot read a device table: checking that the factors are finite is the CALLER's job
 * (meshdqn_amd/inflow.py builds and checks them on the host; no trigonometry runs on the device).
 */
MDQ_API int mdq_ipcs_evolve_inflow(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift,
                    int32_t* iters, const double* inflow_scale, void* stream);

/*
 * mdq_ipcs_reset_history(d, iters) followed by mdq_ipcs_evolve_inflow(...) without the reset launch where the mode allows
 * it (appended within ABI 8).  Mode 3: the three kernels of the launch's FIRST step take the history as empty (no stored
 * tentative velocities, an empty correction ring, no lagged |b|), assign the iteration words instead of adding to them and
 * write the counters they write anyway - one launch and its gap less on the flow chain of every S3 env step.  Every other
 * mode: the reset kernel is launched in front of the evolve kernel, as the two calls would.
 */
MDQ_API int mdq_ipcs_evolve_fresh(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift,
                    int32_t* iters, const double* inflow_scale, void* stream);

/*
 * A NON-SEPARABLE inflow profile u_x(inlet, t) = profile(x, y, t) for the steps of one call (appended within ABI 8): the
 * caller evaluates the profile on the host at every environment's inlet dofs for each step and uploads the table once.
 * All arrays are device arrays; the rows lists come from the cells (meshdqn_amd/inflow.py: inlet_tables, profile_values).
 */
typedef struct mdq_inflow_profile {
  int32_t NIN, NIR;            /* capacities: inlet dofs / inlet-adjacent rows per environment */
  const int32_t* n_inlet;      /* [B] */
  const int32_t* inlet_dofs;   /* [B][NIN]  scalar P2 dofs, padded with -1 */
  const int32_t* n_rows;       /* [B] */
  const int32_t* rows;         /* [B][NIR]  non-Dirichlet P2 rows that share a cell with an inlet dof */
  const double*  values;       /* [B][nsteps][NIN]  x-velocity at inlet_dofs for each step of this call */
} mdq_inflow_profile;

/*
 * mdq_ipcs_evolve under a per-environment inflow profile that need not be separable (the reference's `inflow_profile`
 * evaluated per step, flow_solver.py:366-371, for ANY profile of (x, y, t)).
 *   prof : the tables above.  NULL: exactly mdq_ipcs_evolve.
 * The symmetric elimination is linear in the Dirichlet vector and only the inlet carries non-zero values, so the inflow of
 * a step changes bcu_gx at the inlet dofs and lift1 = A1[:, bc] g, lift3 = M[:, bc] g on the rows that share a cell with
 * an inlet dof - nothing else.  In front of the kernels of step s one small kernel (inflow_lift_kernel, one workgroup per
 * environment) scatters values[b][s] into bcu_gx and recomputes lift1 / lift3 on `rows` from geom, cell_dofs and the flags
 * (which set-up or assembly wrote before); idiag1, sdiagM, geom and every other row stay as they are.  No row of `rows`
 * may be an outflow row (the outflow correction of the lifts is not re-applied; the channel meshes have none).
 * Operator modes 2 and 3 (one launch sequence per step); the modes that loop over the steps inside one kernel (0, 1, 4, 5,
 * 7) return an error before anything is launched.  AFTER the call bcu_gx, lift1 and lift3 of the descriptor hold the LAST
 * step's inflow (what mdq_ipcs_setup_matfree leaves behind for that bcu_gx): a following mdq_ipcs_evolve steps under it.
 * The entry point cannot read a device table: shapes, dof / row ranges and finiteness are the CALLER's job.
 */
MDQ_API int mdq_ipcs_evolve_profile(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift,
                    int32_t* iters, const mdq_inflow_profile* prof, void* stream);

/*
 * The inlet_dofs / rows tables of a mdq_inflow_profile for meshes whose dofs were numbered ON THE DEVICE (the S3 flow leg:
 * a new mesh and a new numbering every env step; appended within ABI 8).  Boundary vertices are never removed or moved and
 * the inlet facets lie on the convex hull, so the inlet POINTS of an environment are those of its original mesh for a whole
 * episode; the caller evaluates its profile at them once, in a canonical order, and this kernel (inlet_map_kernel, one
 * workgroup per environment) finds which dof of the current mesh is which point.
 *   NIN, NIR   : capacities of the lists per environment (NIN <= 64); d->N2 <= 3584 (the meshes of operator mode 3)
 *   n_ref      : device int32[B]       inlet dofs of the canonical inlet
 *   inlet_y    : device double[B][NIN] their y, ascending (meshdqn_amd/inflow.py: canonical_inlet)
 *   n_inlet, inlet_dofs [B][NIN], n_rows, rows [B][NIR] : outputs, laid out as in mdq_inflow_profile; inlet_dofs[b][r] is the
 *                dof whose y has rank r among the inlet dofs, so values[b][s][r] belongs to inlet_y[b][r]; rows ascending;
 *                both padded with -1
 *   map_status : device int32[B], sticky (written only while 0; zero it before the first call): the first failure of an
 *                environment - 1 inlet count != n_ref[b], 2 a y differs from inlet_y by more than 1e-12 (top - bot),
 *                3 more than NIR rows, 4 an inlet-adjacent free row is a row of an outflow facet (mdq_ipcs_evolve_profile
 *                does not re-apply their correction).  A failing environment gets n_inlet = n_rows = 0 and lists of -1 (its
 *                flow then runs under whatever bcu_gx holds: read map_status before trusting its forces); the other
 *                environments are not disturbed, and every write stays inside the lists whatever the mesh data hold.
 * PRECONDITION: bcu_gx is what mdq_env_topology (or the host engine) wrote for this mesh, the constant parabola - the inlet
 * dofs are the dofs with bcu_flag != 0 && bcu_gx != 0 - so call it before the first mdq_ipcs_evolve_profile /
 * mdq_ipcs_evolve_fresh_profile on the mesh, which rewrite bcu_gx.  Reads nv, nt, ne, coords, cell_dofs, cell_outflow,
 * bcu_flag, bcu_gx of the descriptor; needs no set-up and no workspace.
 */
MDQ_API int mdq_ipcs_build_inlet_map(const mdq_ipcs_desc* d, int32_t NIN, int32_t NIR,
                    const int32_t* n_ref, const double* inlet_y,
                    int32_t* n_inlet, int32_t* inlet_dofs, int32_t* n_rows, int32_t* rows, int32_t* map_status, void* stream);

/*
 * mdq_ipcs_evolve_fresh under an inflow profile: mdq_ipcs_evolve_profile on a new mesh in the same descriptor, the history
 * taken as empty the way mdq_ipcs_evolve_fresh does it (appended within ABI 8).  prof = NULL: exactly mdq_ipcs_evolve_fresh
 * with inflow_scale = NULL.  Same argument checks and the same refusal of every operator mode but 2 and 3, before any launch,
 * as mdq_ipcs_evolve_profile.
 */
MDQ_API int mdq_ipcs_evolve_fresh_profile(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift,
                    int32_t* iters, const mdq_inflow_profile* prof, void* stream);

/*
 * Same as mdq_ipcs_evolve (`FlowSolver.evolve`, flow_solver.py:362-396) for the three-kernel mode 3, with HIP events recorded on `stream` around every
 * kernel launch; the accumulated durations (milliseconds over all nsteps) of the velocity / pressure /
 * correction kernels are returned in host array kernel_ms[3].  Synchronises the stream (measurement aid).
 */
MDQ_API int mdq_ipcs_evolve_timed(const mdq_ipcs_desc* d, int32_t nsteps, double* drag, double* lift,
                          int32_t* iters, void* stream, double* kernel_ms);

/*
 * Drag and lift of given fields on every environment's current mesh.
 * Replaces `DragProbe.sample(u,p)` / `LiftProbe.sample(u,p)` (probes.py:23-50)
 * as used by `Env2DAirfoil.calculate_reward` (Env2DAirfoil.py:390-394).
 *   u : device double[B][nfields][N2][2], p : device double[B][nfields][NV]
 *   drag, lift : device double[B][nfields]
 */
MDQ_API int mdq_probe_forces(const mdq_ipcs_desc* d, int32_t nfields, const double* u, const double* p,
                     double* drag, double* lift, void* stream);

/*
 * The factorisation half of `LUSolver("mumps")` (flow_solver.py:150-159; repeated by the reference for every
 * coarsened mesh, :318-328) on the device: builds the substructuring factors pd_* of every environment's scaled,
 * boundary-eliminated pressure matrix (K1s, as written by mdq_ipcs_assemble / mdq_ipcs_setup_matfree) - recursive
 * coordinate bisection into 8 parts, vertex separator, dense inverses of the interior blocks and of the Schur
 * complement by Gauss-Jordan in LDS.  The pd_* arrays of `d` must be allocated with capacities NPART >= 8,
 * NPW >= 8 * 112^2, NPF >= 8 * 112 * 48, NPGI >= 8 * 48, NPS >= 112^2 + 8 * 48^2 (the inverse Schur complement in front, one 48^2 scratch slice per subdomain behind it: an
 * environment with fewer subdomains is accepted with less, see -2 below), NPGK >= 112 * 16 (written here although the
 * descriptor declares them const: they are this call's outputs).  status (device int32 [B], may be NULL): 0 ok;
 * < 0: the mesh exceeds those limits - its header says nparts = 0 and mdq_ipcs_evolve (pd_enabled = 1) runs the
 * Krylov pressure solve for that environment.  The codes, in the order they are checked, each for ONE environment:
 *   -1  nv outside [1, 1024] (nothing but the header and the status is written);
 *   -2  a subdomain with more than 112 interior nodes, more than 112 separator nodes, more subdomains than NPART, or
 *       NPS < 112^2 + 48^2 * (its number of subdomains);
 *   -3  more entries of K[G, I] than NPGK;
 *   -4  a subdomain touching more than 48 separator nodes, or its blocks beyond NPW / NPF / NPGI.
 * A refused environment may have written part of its own [b] slices of the pd_* arrays, never another one's.
 */
MDQ_API int mdq_ipcs_factorize_pressure(const mdq_ipcs_desc* d, int32_t* status, void* stream);

/* ---- graph Q-network forward (airfoilgcnn.py:85-145 NodeRemovalNet, :170-209 AirfoilGCNN) ---- */
typedef struct mdq_gcn_level {
  int32_t type;          /* 0 = SAGEConv (mean aggr, root weight), 1 = GCNConv (self loops, sym. norm) */
  int32_t fin;           /* input features of this level */
  const float* w_l;      /* device [fin][C]: SAGE lin_l.weight^T / GCN lin.weight^T */
  const float* b;        /* device [C]: SAGE lin_l.bias / GCN bias */
  const float* w_r;      /* device [fin][C]: SAGE lin_r.weight^T (unused for GCN) */
  const float* pool_w;   /* device [C]: TopKPooling.weight */
} mdq_gcn_level;

typedef struct mdq_gcn_net {
  int32_t nlevels, C, fin0, out_dim;  /* conv/pool levels, conv width, input features, head outputs */
  double ratio;                       /* TopKPooling ratio */
  int32_t softmax;                    /* 1: softmax over the head outputs (NodeRemovalNet, head "softmax") */
  int32_t dueling;                    /* 1: dueling aggregation of the head outputs (see lin_v_w below); excludes softmax.
                                         Both 0: the raw lin3 outputs (AirfoilGCNN; NodeRemovalNet, head "linear") */
  mdq_gcn_level levels[6];
  const float* lin1_w;   /* device [2C][128]  lin1.weight^T */
  const float* lin1_b;
  const float* lin2_w;   /* device [128][64] */
  const float* lin2_b;
  const float* lin3_w;   /* device [64][out_dim] */
  const float* lin3_b;
  /* optional, appended within ABI 8 (read only when dueling != 0): the value stream of the dueling head (Wang et al.
     2016; not a reference feature).  With a2 = relu(lin2(relu(lin1(emb)))), A = lin3(a2) and v = lin_v_b + a2 . lin_v_w the
     outputs of a graph are q_c = v + (A_c - mean_j A_j).  `dueling` takes the place of the padding word behind `softmax`
     and the two pointers are the struct's last fields, so MDQ_ABI_VERSION stays 8: zero-initialised they mean what ABI 8
     meant, and a caller that zero-initialises the descriptor (every ABI 8 caller must) and is rebuilt against this header
     behaves as before; no entry point or exported symbol is added.  mdq_gcn_forward* and mdq_gcn_train_step* refuse, before
     any launch, dueling together with softmax and dueling with either pointer NULL. */
  const float* lin_v_w;  /* device [64]  lin_v.weight */
  const float* lin_v_b;  /* device [1] */
} mdq_gcn_net;

/*
 * Batched forward of B graphs (one workgroup per graph, whole network out of LDS; dense head on MFMA).
 * Replaces `NodeRemovalNet.forward(Batch)` (airfoilgcnn.py:85-145) / `AirfoilGCNN.forward(Batch)` (airfoilgcnn.py:170-209)
 * and the PyG layers they call (SAGEConv / GCNConv / TopKPooling / global max + mean pool, airfoilgcnn.py:30-41).
 *   x        device float [sum_nodes][fin0]     node features, graphs concatenated
 *   node_ptr device int32 [B+1]                 first node of every graph
 *   esrc/edst device int32 [sum_edges]          edge end points, LOCAL node ids (0..n_g-1), j -> i
 *   edge_ptr device int32 [B+1]
 *   emb      device float [B][2C]  (out)        graph embeddings (x1+x2+...)
 *   out      device float [B][out_dim] (out)    head outputs (softmax probabilities if net.softmax, dueling q if net.dueling)
 *   NMAX / EMAX: upper bounds of nodes / edges per graph (sizes the LDS carve-up)
 */
MDQ_API int mdq_gcn_forward(const mdq_gcn_net* net, int32_t B, int32_t NMAX, int32_t EMAX, const float* x,
                    const int32_t* node_ptr, const int32_t* esrc, const int32_t* edst,
                    const int32_t* edge_ptr, float* emb, float* out, void* stream);

/*
 * The same forward with two optional device outputs (either may be NULL):
 *   perm   int32 [B][nlevels][NMAX]  TopKPooling's `perm` of every level (airfoilgcnn.py:96: kept node r of level l =
 *                                    node perm[r] of the level's input; entries past ceil(ratio n) are -1) - the INDEX
 *                                    work of the Q-path, which the parity tests hold bit-exact against the oracle
 *   status int32 [B]                 0 ok, -1 / -2: graph b has more nodes / edges than NMAX / EMAX (its outputs are NaN;
 *                                    the LDS carve-up is sized from those bounds, a larger graph is never staged)
 */
MDQ_API int mdq_gcn_forward_ex(const mdq_gcn_net* net, int32_t B, int32_t NMAX, int32_t EMAX, const float* x,
                       const int32_t* node_ptr, const int32_t* esrc, const int32_t* edst,
                       const int32_t* edge_ptr, float* emb, float* out, int32_t* perm, int32_t* status, void* stream);

/* The same forward on edge lists PADDED to EMAX slots per graph (graph b: esrc_pad / edst_pad [b * EMAX .. + edge_cnt[b])) -
 * the layout mdq_env_topology writes (edge_src / edge_dst / nedges): no offsets, no compaction in front of the Q-forward
 * of a device-resident env step. */
MDQ_API int mdq_gcn_forward_padded(const mdq_gcn_net* net, int32_t B, int32_t NMAX, int32_t EMAX, const float* x,
                           const int32_t* node_ptr, const int32_t* esrc_pad, const int32_t* edst_pad,
                           const int32_t* edge_cnt, float* emb, float* out, int32_t* perm, int32_t* status, void* stream);

/* ---- the learning step of the graph Q-network (airfoil_dqn.py:240-310 DataWorker.compute_gradients) ---- */
/* Offsets (in floats) of every trained parameter inside the flat gradient: the parameters of the module in
 * `parameters()` order, each in torch layout [out][in] - the message of the gradient all-reduce. */
typedef struct mdq_gcn_grad_layout {
  int32_t w_l[6], b[6], w_r[6], pool_w[6]; /* per level: lin_l.weight | lin.weight, lin_l.bias | bias, lin_r.weight (SAGE), pool weight */
  int32_t lin1_w, lin1_b, lin2_w, lin2_b, lin3_w, lin3_b;
  int32_t total;                           /* floats of the flat gradient (ALL parameters of the module) */
  int32_t lin_v;                           /* dueling head only (read when net.dueling != 0; took the place of the padding
                                              word): offset of lin_v.weight [64], its bias sits at lin_v + 64 */
} mdq_gcn_grad_layout;

typedef struct mdq_gcn_train_desc {
  int32_t B, NMAX, EMAX;   /* graphs of the minibatch; bounds of nodes / edges per graph (size the LDS carve-up) */
  int32_t mode;            /* which side of the double-DQN loss this network is on (the reference's `select` toggle):
                              0: loss_b = huber(out[b][action_b] - (reward_b + gamma nonfinal_b max_j q_other[b][j]))
                              1: loss_b = huber(q_other[b][action_b] - (reward_b + gamma nonfinal_b max_j out[b][j])) */
  double gamma;
  const float* x;          /* graphs as for mdq_gcn_forward: the states (mode 0) / the next states (mode 1) */
  const int32_t* node_ptr;
  const int32_t* esrc;
  const int32_t* edst;
  const int32_t* edge_ptr;
  const float* q_other;    /* device [B][out_dim] outputs of the OTHER network (no gradient): on the next states (mode 0) / the states (mode 1) */
  const int64_t* action;   /* device [B] */
  const float* reward;     /* device [B] */
  const float* nonfinal;   /* device [B] 1 where the transition has a next state, else 0 */
  float* workspace;        /* device [B][mdq_gcn_train_workspace()] floats of scratch */
  float* partial;          /* device [B][layout.total]: per-graph gradients; zero-filled ONCE by the caller (the slots of
                              parameters the forward never uses are never written and must read 0) */
  float* grad;             /* device [layout.total] (out): flat gradient of the mean loss */
  float* loss;             /* device [1] (out): mean Huber loss (delta 1) over the minibatch */
  float* out;              /* device [B][out_dim] (out, may be NULL): head outputs of this network */
  mdq_gcn_grad_layout layout;
} mdq_gcn_train_desc;

/* floats of workspace per graph for mdq_gcn_train_step (-1: bad arguments) */
MDQ_API int64_t mdq_gcn_train_workspace(const mdq_gcn_net* net, int32_t NMAX, int32_t EMAX);

/*
 * Forward + double-DQN Huber loss + full backward of `net` over a minibatch, without autograd: replaces
 * `loss.backward()` in DataWorker.compute_gradients (airfoil_dqn.py:286-310) and the PyG backward passes of SAGEConv /
 * GCNConv / TopKPooling / global max + mean pool behind it.  One workgroup per graph (forward out of LDS, backward over
 * the rows TopKPooling kept), then a reduction of the per-graph gradients in graph order: bitwise reproducible.
 * `out` of the formulas above is what the head puts out: probabilities (net.softmax), the raw lin3 outputs, or the dueling
 * q = v + (A - mean A) (net.dueling).  Dueling backward, g = d loss / d q[j]: d A[c] = g ((c == j) - 1 / out_dim), d v = g;
 * lin_v's gradient goes to layout.lin_v (weight, 64 floats) and layout.lin_v + 64 (bias), which must lie inside `total`.
 */
MDQ_API int mdq_gcn_train_step(const mdq_gcn_net* net, const mdq_gcn_train_desc* d, void* stream);

/*
 * The same learning step with two optional per-graph device arrays (appended within ABI 8; both NULL: exactly
 * mdq_gcn_train_step, which calls this one):
 *   weight float [B] (in)   importance weight w_b of graph b (prioritized replay): its loss term is w_b huber(diff_b), the
 *                           derivative handed to the backward pass is a clamp(diff_b, -1, 1) / B * w_b, `loss` is the mean of
 *                           the weighted terms.  Both are one multiplication behind the unweighted arithmetic: a table of
 *                           ones gives the bits of NULL; a graph of weight 0 leaves an all-zero slice of `partial`.
 *   td     float [B] (out)  diff_b, the TD error the Huber loss is taken of: out[b][action_b] - target_b (mode 0),
 *                           q_other[b][action_b] - target_b (mode 1); NaN for a graph beyond NMAX / EMAX.
 */
MDQ_API int mdq_gcn_train_step_weighted(const mdq_gcn_net* net, const mdq_gcn_train_desc* d, const float* weight, float* td,
                                void* stream);

/* Parameters of the module (torch layout) into the layout the kernels read, all segments in ONE launch:
 * segment s is a [rows][cols] matrix written transposed ([cols][rows]); cols == 1: a plain copy of `rows` floats. */
#define MDQ_GCN_PACK_MAX 32
typedef struct mdq_gcn_pack_table {
  int32_t n, _pad;
  const float* src[MDQ_GCN_PACK_MAX];
  float* dst[MDQ_GCN_PACK_MAX];
  int32_t rows[MDQ_GCN_PACK_MAX], cols[MDQ_GCN_PACK_MAX];
} mdq_gcn_pack_table;
MDQ_API int mdq_gcn_pack(const mdq_gcn_pack_table* table, void* stream);

/* ---- device-resident replay memory + optimiser update (airfoil_dqn.py:48-67 ReplayMemory, :184-200 apply_gradients) ---- */
/*
 * Transition records (float32; the layout trainer.pack_transitions writes and the ranks all-gather), N*F = nf, EM edge slots:
 *   [ x(s) nf | x(s') nf | src(s) EM | dst(s) EM | src(s') EM | dst(s') EM | edges(s) | edges(s') | action | reward | done ]
 * rec_len = 2 nf + 4 EM + 5; a terminal transition has zeros for s'.
 *
 * mdq_replay_step: `ReplayMemory.push` for the B environments of a batched step, in two halves, because the state arrays
 * of the vector environment are rewritten by the next step: the CURRENT batched state (x [B][nf], padded edge lists
 * [B][EM] + nedges [B], as VecEnv2DAirfoil hands them out) becomes s of the records (base_cur + b) % capacity and s' of
 * the records (base_prev + b) % capacity, whose action / reward / done [B] (of the step that led to this state) are
 * filled in too.  base_cur or base_prev < 0: that half is skipped.  All pointers device.
 */
MDQ_API int mdq_replay_step(float* ring, int32_t rec_len, int32_t capacity, int32_t B, int32_t nf, int32_t EM, const float* x,
                    const int32_t* edge_src, const int32_t* edge_dst, const int32_t* nedges, int32_t base_cur,
                    int32_t base_prev, const int32_t* action, const double* reward, const uint8_t* done, void* stream);

/*
 * `ReplayMemory.sample` + the batching of DataWorker._get_data (airfoil_dqn.py:63-64,240-262): records idx[0..n) of the
 * ring -> the graph arrays of mdq_gcn_forward / mdq_gcn_train_step for the states (`_s`) and the next states (`_n`; a
 * terminal transition contributes its own state as a placeholder, nonfinal = 0), edge lists packed back to back.
 */
typedef struct mdq_replay_sample_desc {
  int32_t n, rec_len, nf, EM;
  const float* R;             /* ring */
  const int32_t* idx;         /* [n] record numbers */
  float* x_s;                 /* [n][nf] */
  float* x_n;
  int32_t* esrc_s;            /* [n * EM] packed */
  int32_t* edst_s;
  int32_t* esrc_n;
  int32_t* edst_n;
  int32_t* edge_ptr_s;        /* [n + 1] */
  int32_t* edge_ptr_n;
  int64_t* action;            /* [n] */
  float* reward;              /* [n] */
  float* nonfinal;            /* [n] */
} mdq_replay_sample_desc;
MDQ_API int mdq_replay_sample(const mdq_replay_sample_desc* d, void* stream);

/*
 * The same sampling launch with the n-step transition of every draw composed on the way (appended within ABI 8; ns NULL:
 * exactly mdq_replay_sample, which calls this one; no reference counterpart: its targets are 1-step).  The ring is written
 * in groups of W records, one per batched step, so record (j + W) % capacity is the next transition of the environment of
 * record j.  The walk of draw i takes j_0 = idx[i] and, after taking j_k, stops if k + 1 == n_step, if record j_k is
 * terminal (done > 0.5) or if (j_k + W) % capacity lies in [head, head + W) - the group being written; otherwise
 * j_(k+1) = (j_k + W) % capacity.  With m records taken, L = j_(m-1), g_0 = 1, g_(k+1) = g_k gamma:
 *     x_s, edges of s, action   of record j_0 (as mdq_replay_sample)
 *     reward[i]   = (float) sum_{k<m} g_k (double) reward_(j_k): fp64, in the order k = 0 .. m - 1, every product and every
 *                   sum rounded on its own, rounded to float once
 *     nonfinal[i] = 0 if record L is terminal, else (float) g_(m-1): gamma^m is formed as float(gamma^(m-1)) * float(gamma)
 *                   inside the learning step, which multiplies `nonfinal` by its own gamma; no division: gamma = 0 is served
 *     x_n, edges of s'          s' of record L; L terminal: the own state of j_0 as the masked placeholder
 *     steps[i]    = m
 * Every successor is formed modulo `capacity`: given idx[i] in [0, capacity) (the caller's job, as in mdq_replay_sample) no
 * read leaves the ring whatever it holds.  A drawn record of the head group is taken as it is.  n_step = 1: the bits of
 * mdq_replay_sample for any W, head and gamma.  One launch, no atomics, no device random numbers: run-to-run identical.
 * n_step outside 1 .. 64, W < 1, a capacity that is no multiple of W or below 2 W, a head that is no multiple of W or
 * outside [0, capacity) and a gamma that is negative or not finite are refused before any launch.
 */
typedef struct mdq_replay_nstep {
  int32_t n_step;             /* 1 .. 64 */
  int32_t W;                  /* records per group: the successor of record j is (j + W) % capacity */
  int32_t capacity;           /* records of the ring, a multiple of W, at least 2 W */
  int32_t head;               /* first record of the group the walk must never step INTO: the group being written
                                 (SharedDeviceReplay.group_base(t)); a multiple of W in [0, capacity) */
  double gamma;               /* finite, >= 0 */
  int32_t* steps;             /* device [n] (out, may be NULL): m_i, the transitions composed for draw i */
} mdq_replay_nstep;
MDQ_API int mdq_replay_sample_nstep(const mdq_replay_sample_desc* d, const mdq_replay_nstep* ns, void* stream);

/*
 * Proportional prioritized replay on the record ring (Schaul et al. 2016; no reference counterpart: ReplayMemory.sample is
 * uniform).  Appended within ABI 8.  float prio[capacity] holds p_j = (|td_j| + eps)^alpha of record j, and
 *     prio[j] == 0  <=>  record j must not be drawn (never written, or of the group that is being written),
 * so no entry point takes a window.  float pmax[1] is the largest priority seen so far (the caller starts it at 1).  All
 * pointers device; every launch on `stream`; no atomics, no device random numbers: results are run-to-run identical.
 *
 * mdq_replay_prio_fill: prio[(base_new + i) % capacity] = *pmax for i < n_new (a group whose records have just received
 * their next states: every new transition is drawn at least once soon) and prio[(base_zero + i) % capacity] = 0 for
 * i < n_zero (the group about to be written).  Either length may be 0 (both: no launch).  A range longer than the
 * capacity, a base outside [0, capacity) and ranges that overlap are refused before any launch.
 */
MDQ_API int mdq_replay_prio_fill(float* prio, int32_t capacity, int32_t base_new, int32_t n_new, int32_t base_zero,
                         int32_t n_zero, const float* pmax, void* stream);

/*
 * mdq_replay_prio_draw: one stratified minibatch of n records, one workgroup.  With S_j = prio[0] + ... + prio[j] (fp64,
 * summed in an order that depends on `capacity` only) and total = S_{capacity - 1}:
 *     t_i       = total * ((i + u[i]) / n)                     evaluated as written, in fp64
 *     idx[i]    = the smallest j with S_j > t_i (such a record has prio[j] > 0); if there is none - (i + u[i]) / n rounded
 *                 to 1 - the last j with prio[j] > 0
 *     weight[i] = (float) pow(min_k prio[idx[k]] / prio[idx[i]], beta)      (fp64, rounded once): the importance weights
 *                 (N p_i)^-beta divided by their largest one
 *     total[0]  = total                                        (if `total` is not NULL)
 * total == 0 (nothing to draw from): every idx[i] = 0 and every weight[i] = 0 - nothing downstream reads out of bounds and
 * the minibatch carries no gradient.
 */
typedef struct mdq_replay_prio_draw_desc {
  int32_t capacity, n;        /* records of the ring; draws, 1 .. 1024 */
  double beta;                /* >= 0 */
  const float* prio;          /* [capacity] */
  const double* u;            /* [n] uniforms in [0, 1), drawn by the host */
  int32_t* idx;               /* [n] (out) */
  float* weight;              /* [n] (out) */
  double* total;              /* [1] (out, may be NULL) */
} mdq_replay_prio_draw_desc;
MDQ_API int mdq_replay_prio_draw(const mdq_replay_prio_draw_desc* d, void* stream);

/*
 * mdq_replay_prio_update: for i = 0 .. n - 1 in this order (n <= 1024; one workgroup), unless td[i] is not finite (a graph
 * the learning step refused) or idx[i] lies outside [0, capacity):
 *     v = (float) pow(|td[i]| + eps, alpha)  (fp64, rounded once);   prio[idx[i]] = v;   *pmax = max(*pmax, v)
 * - so among several draws of one record the last one stays.  No write ever leaves the array.
 */
MDQ_API int mdq_replay_prio_update(float* prio, int32_t capacity, int32_t n, const int32_t* idx, const float* td, double alpha,
                           double eps, float* pmax, void* stream);

/*
 * torch.optim.Adam.step (amsgrad False; weight decay added to the gradient) for up to 32 parameter tensors in one
 * launch: segment s updates param[s][0..len[s]) from grad / exp_avg / exp_avg_sq [offset[s] ..] (flat buffers laid out
 * like the flat gradient).  bias_correction{1,2} = 1 - beta{1,2}^step, computed by the caller.  Per element, in float:
 *     g' = g + wd p  (only if wd != 0);   m' = m + w1 (g' - m);   v' = b2 v + w2 (g' g');
 *     p' = p - lr_c (m' / (sqrt(v') / bc2s + eps))
 * with w1 = 1 - beta1, w2 = 1 - beta2, lr_c = lr / bias_correction1 and bc2s = sqrt(bias_correction2) formed in double and
 * rounded once to float (as torch forms them), and b2, eps, wd the doubles rounded once.  The operations are the ones above
 * in that order; a product and the sum that takes it may be contracted into one fused multiply-add, sqrt and the divisions
 * are correctly rounded.  grad is only read; nothing outside the n segments is written.  A segment with len 0 is skipped
 * whatever its pointer.  Refused before any launch (nonzero return, mdq_last_error names mdq_adam_step and the field): n
 * outside 1 .. 32; grad, exp_avg or exp_avg_sq NULL; among the first n segments a negative len, a negative offset, offset +
 * len beyond int32, or param NULL where len > 0; lr, eps or weight_decay negative or not finite; beta1 or beta2 outside
 * [0, 1); bias_correction1 or bias_correction2 outside (0, 1].
 */
typedef struct mdq_adam_desc {
  int32_t n, _pad;
  float* param[MDQ_GCN_PACK_MAX];
  int32_t offset[MDQ_GCN_PACK_MAX], len[MDQ_GCN_PACK_MAX];
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  double lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2;
} mdq_adam_desc;
MDQ_API int mdq_adam_step(const mdq_adam_desc* d, void* stream);

/*
 * Target network and Double-DQN targets (Mnih et al. 2015, van Hasselt et al. 2016; no reference counterpart: its two
 * networks swap roles every `target_update` steps and never exchange weights).  Appended within ABI 8.  Two launches of the
 * optimiser chain around the unchanged learning step; all pointers device; no atomics, no device random numbers: results
 * are run-to-run identical.
 *
 * mdq_double_q_select: q_online, q_target and q_sel are float [B][OUT], sel is int32 [B] and may be NULL.  Per row b, with
 * best = -inf and j* = 0, for j = 0 .. OUT - 1 in this order: q_online[b][j] replaces the pair only if it is > best - the
 * first maximum wins (torch.argmax; -0 and +0 are equal), a NaN is never selected, a row with nothing above -inf gives
 * j* = 0.  Then
 *     v = q_target[b][j*];   q_sel[b][c] = v for every c < OUT;   sel[b] = j*
 * - the row is broadcast, so `max_j q_other[b][j]` of mdq_gcn_train_step in mode 0 with q_other = q_sel is exactly v: the
 * target r + gamma nonfinal Q_target(s', argmax_a Q_online(s', a)) without a change to the learning step.  One launch, one
 * wave per row, MDQ_DOUBLE_Q_ROWS rows per workgroup, any OUT >= 1.  q_online and q_target may be the same array (v is then
 * the row's maximum).  B <= 0, OUT <= 0, a NULL among the three arrays and a q_sel that overlaps q_online or q_target are
 * refused before any launch.
 */
#define MDQ_DOUBLE_Q_ROWS 4
MDQ_API int mdq_double_q_select(int32_t B, int32_t OUT, const float* q_online, const float* q_target, float* q_sel,
                        int32_t* sel, void* stream);

/*
 * mdq_target_update: the target network's parameters follow the online ones, up to 32 parameter tensors in one launch
 * (tensor s: len[s] floats; the grid of mdq_adam_step).  tau == 1: dst[s][i] = src[s][i], the bits (NaN payloads and the
 * sign of zero included).  Otherwise, with tf = (float) tau,
 *     dst[s][i] = dst[s][i] + tf * (src[s][i] - dst[s][i])
 * in three float operations, each rounded on its own (no fused multiply-add): a float32 restatement gives the same bits.
 * n outside 1 .. 32, a NULL pointer or a negative len among the first n, a tau that is not finite or outside (0, 1] and
 * dst[s] == src[s] are refused before any launch.
 */
typedef struct mdq_target_update_desc {
  int32_t n, _pad;
  float* dst[MDQ_GCN_PACK_MAX];
  const float* src[MDQ_GCN_PACK_MAX];
  int32_t len[MDQ_GCN_PACK_MAX];
  double tau;                 /* in (0, 1] */
} mdq_target_update_desc;
MDQ_API int mdq_target_update(const mdq_target_update_desc* d, void* stream);

/*
 * Noisy-network exploration (Fortunato et al. 2018, factorised Gaussian noise on the dense head; no reference counterpart:
 * its exploration is epsilon-greedy).  Appended within ABI 8.  The fused forward and the learning step read the PACKED copy
 * of the parameters, so the noise is added while packing and neither of them changes.  All pointers device; no atomics.
 *
 * mdq_gcn_pack_noisy: mdq_gcn_pack with n = 1 .. MDQ_NOISY_MAX noisy layers, in ONE launch of the same grid.  A table
 * segment that `nz` does not name is packed exactly as mdq_gcn_pack packs it.  Noisy layer L names its weight segment seg_w[L]
 * (a transposed one: rows = out, cols = in) and its bias segment seg_b[L] (rows = out, cols = 1), sigma_w[L] float
 * [out][in], sigma_b[L] float [out] and two OUTPUT vectors eps_in[L] float [in], eps_out[L] float [out].  It writes
 *     dst_w[i * out + o] = mu_w[o][i] + sigma_w[o][i] * (eps_out[o] * eps_in[i])
 *     dst_b[o]           = mu_b[o]    + sigma_b[o]    * eps_out[o]
 * in float, in exactly these operations and this order, each rounded on its own (no fused multiply-add): a float32
 * restatement from the eps vectors the launch wrote gives the same bits.
 *
 * The noise is counter-based, nothing comes from the host and no workgroup waits for another: entry j of side s (0 = in,
 * 1 = out) of layer L is Philox4x32-10 (Salmon et al. 2011) with key (seed, stream) and counter (j, 2 L + s, draw_lo,
 * draw_hi); of its output words r0, r1
 *     u1 = ((r0 >> 8) + 1) * 2^-24   in (0, 1]        u2 = (r1 >> 8) * 2^-24   in [0, 1)
 *     z  = sqrtf(-2 logf(u1)) * cospif(2 u2)          eps = copysignf(sqrtf(|z|), z)
 * - the float functions are logf, sqrtf (correctly rounded) and cospif, whose argument 2 u2 is exact, so z keeps its
 * relative accuracy where the cosine passes through zero.  Every workgroup recomputes the eps values its tile needs; the
 * first workgroup of a layer's weight segment also stores the two vectors.  The same (seed, stream, draw) gives the same
 * bits on every run, and |eps| <= sqrt(sqrt(48 ln 2)) < 2.41 always (u1 >= 2^-24).
 *
 * mdq_noisy_grad: the gradient of the sigmas from the gradient of the means the learning step wrote into the flat
 * gradient `grad` (lay->total floats), one launch:
 *     grad[sig_w[L] + o * in + i] = grad[mu_w[L] + o * in + i] * (eps_out[o] * eps_in[i])
 *     grad[sig_b[L] + o]          = grad[mu_b[L] + o] * eps_out[o]
 * with out = lay->out[L], in = lay->in[L], the same float product as the pack, read from the eps vectors of `nz` (of which
 * it uses n and those pointers only).
 *
 * Refused before any launch (nonzero return, mdq_last_error names the entry point and the field): a NULL argument; n
 * outside 1 .. 4; among the first n layers a NULL sigma or eps pointer; for the pack a bad table (n outside 1 .. 32), a
 * segment index outside the table, a segment named twice, a weight segment with rows or cols < 1, a bias segment whose
 * rows differ from the weight segment's or whose cols are not 1; for the gradient out or in < 1, a slice outside
 * [0, total) and two slices (of any layers) that overlap.
 */
#define MDQ_NOISY_MAX 4
typedef struct mdq_noisy_desc {
  int32_t n, _pad;
  uint32_t seed, stream;        /* the Philox key */
  uint64_t draw;                /* counter words 2 (low half) and 3 */
  int32_t seg_w[MDQ_NOISY_MAX], seg_b[MDQ_NOISY_MAX];
  const float* sigma_w[MDQ_NOISY_MAX];
  const float* sigma_b[MDQ_NOISY_MAX];
  float* eps_in[MDQ_NOISY_MAX];
  float* eps_out[MDQ_NOISY_MAX];
} mdq_noisy_desc;
typedef struct mdq_noisy_grad_layout {
  int32_t total, _pad;
  int32_t out[MDQ_NOISY_MAX], in[MDQ_NOISY_MAX];
  int32_t mu_w[MDQ_NOISY_MAX], mu_b[MDQ_NOISY_MAX], sig_w[MDQ_NOISY_MAX], sig_b[MDQ_NOISY_MAX];
} mdq_noisy_grad_layout;
MDQ_API int mdq_gcn_pack_noisy(const mdq_gcn_pack_table* table, const mdq_noisy_desc* nz, void* stream);
MDQ_API int mdq_noisy_grad(const mdq_noisy_desc* nz, const mdq_noisy_grad_layout* lay, float* grad, void* stream);

/* Up to 8 buffer copies in one launch (no reference counterpart; the env step hands its meshes and the warm-start fields
 * to the flow engine with it): buffer t = rows[t] rows of row_bytes[t] bytes, consecutive rows src_stride_bytes[t] /
 * dst_stride_bytes[t] apart (all multiples of 4, pointers 4-byte aligned; device pointers, host arrays of them). */
MDQ_API int mdq_copy_strided(int32_t n, void* const* dst, const void* const* src, const int64_t* rows, const int64_t* row_bytes,
                     const int64_t* src_stride_bytes, const int64_t* dst_stride_bytes, void* stream);

/* Probe kernel for meshdqn_amd/streams.py (no reference counterpart): `wgs` workgroups that each hold `lds_bytes` of LDS and
 * spin for `ticks_100mhz` ticks of the 100 MHz wall clock - with more workgroups than CUs it keeps the dispatcher of its
 * hardware queue busy, which is how two HIP streams are tested for really running beside each other. */
MDQ_API int mdq_spin(int32_t wgs, int32_t lds_bytes, int64_t ticks_100mhz, void* stream);

/* A HIP stream restricted to the compute units of `mask` (nwords 32-bit words; bit i = compute unit i in the driver's
 * numbering, which goes round-robin over the XCDs and then over the shader engines of an XCD), and its release.  No
 * reference counterpart: meshdqn_amd/streams.py gives the env step's main chain and its flow leg disjoint halves of the
 * chip (both are chains of kernels with one workgroup per environment). */
MDQ_API int mdq_stream_create_cu_mask(const uint32_t* mask, int32_t nwords, void** stream);
MDQ_API int mdq_stream_destroy(void* stream);

/* ---- snapshot interpolation onto coarsened meshes (Env2DAirfoil.py:556-593, :515-522) ---- */
/* ABI 8: one source (original mesh + its snapshots + its location grid) of a batch that mixes several airfoils - the
 * source fields of mdq_interp_desc in one record; a DEVICE array of these is mdq_interp_desc.srcs. */
typedef struct mdq_interp_src {
  int32_t src_nv, src_nt, src_n2;
  int32_t gnx, gny;
  int32_t _pad;
  double x0, y0, inv_hx, inv_hy;
  const double* src_coords;     /* [src_nv][2]       (device, as in mdq_interp_desc) */
  const int32_t* src_cell_dofs; /* [6][src_nt]                                     */
  const double* src_geom;       /* [5][src_nt]                                     */
  const int32_t* bin_ptr;       /* [gnx*gny+1]                                     */
  const int32_t* bin_cells;
  const double* src_u;          /* [S][src_n2][2]                                  */
  const double* src_p;          /* [S][src_nv]                                     */
  const double* src_cellrec;    /* [src_nt][6] or NULL                             */
} mdq_interp_src;

typedef struct mdq_interp_desc {
  int32_t B, S;            /* target meshes (environments), snapshots                         */
  int32_t NP, NP1;         /* capacities: target P2 points (vertices then edge midpoints), P1 points (vertices) */
  int32_t src_nv, src_nt, src_n2;
  int32_t gnx, gny;        /* uniform location grid over the source mesh                       */
  int32_t _pad;
  double x0, y0, inv_hx, inv_hy;
  const int32_t* npts;     /* device [B]   P2 target points per environment                    */
  const int32_t* np1;      /* device [B]   P1 target points (= vertices) per environment       */
  const double* points;    /* device [B][NP][2]  target coordinates                            */
  /* source (original, smoothed) mesh and its snapshots, device */
  const double* src_coords;     /* [src_nv][2]                                                 */
  const int32_t* src_cell_dofs; /* [6][src_nt]                                                 */
  const double* src_geom;       /* [5][src_nt] as written by mdq_ipcs_assemble                 */
  const int32_t* bin_ptr;       /* [gnx*gny+1] candidate cells per grid bin (ascending ids, never empty) */
  const int32_t* bin_cells;
  const double* src_u;          /* [S][src_n2][2]                                              */
  const double* src_p;          /* [S][src_nv]                                                 */
  /* outputs, device */
  double* out_u;                /* [B][S][NP][2]                                               */
  double* out_p;                /* [B][S][NP1]                                                 */
  int32_t* out_cell;            /* [B][NP] located source cell (may be NULL)                   */
  /* optional, device: [src_nt][6] = {x, y of the cell's vertex 0, the four Jinv entries of src_geom} - what the point
   * location needs of a candidate cell in ONE record, 16-byte aligned (NULL: gathered from src_cell_dofs / src_coords /
   * src_geom) */
  const double* src_cellrec;
  /* optional, device [B]: added to npts[b] (a caller that holds vertex and edge counts separately passes np1 as npts and
   * the edge counts here instead of launching an add) */
  const int32_t* npts_extra;
  /* optional (ABI 5, round 4), `sparse` != 0: only what the device-resident env step reads of the S x (P2 + P1) fields -
   *   vertices: every snapshot (state features, pressures of the force integrals);
   *   edge midpoints: the LAST snapshot only (the warm start of the flow leg; sparse = 2: not even that - a step without
   *   a flow leg), and every snapshot for the three edges of the cells that carry an airfoil facet (the force integrals of
   *   the reward, probes.py:23-50).  The other entries of out_u keep whatever they held.  Needs the topology engine's
   *   airfoil-facet list and cell dofs of the TARGET meshes. */
  const int32_t* af_facets;     /* device [B][NAF][2] (cell, local facet)                      */
  const int32_t* naf;           /* device [B]                                                  */
  const int32_t* cell_dofs;     /* device [B][6][NT] dof ids of the target meshes              */
  int32_t NT, NAF;
  int32_t sparse, _pad2;
  /* optional (ABI 8): per-environment sources of a batch over n_src airfoils.  srcs (device [n_src]) and src_of_env
   * (device [B], values in [0, n_src)) both set: environment b is interpolated from srcs[src_of_env[b]] and the source
   * fields above (src_nv .. src_p, src_cellrec, the grid) are ignored; both NULL: the one shared source above. */
  int32_t n_src, _pad3;
  const int32_t* src_of_env;
  const mdq_interp_src* srcs;
} mdq_interp_desc;

/*
 * Interpolate S stored (u, p) snapshots of the ORIGINAL mesh onto the P2 / P1 dof points of B
 * coarsened meshes: point location (containing cell) + basis evaluation.
 * Replaces `v_func.interpolate(original_u)` / `p_func.interpolate(original_p)` (Env2DAirfoil.py:556-568).
 * A point in no cell is extrapolated from the least violated candidate of its grid bin (bin-local: the bin
 * clamped to the grid outside the grid's box, the nearest-centroid cell in an empty bin), not from the mesh's
 * closest cell.  The environment only meets round-off cases: over the P2 dof points of both golden episodes
 * (295 248 points) 1.4 % lie in no cell, each by at most 1.9e-15 in barycentric coordinates (points on shared
 * or boundary edges).  out_cell[b][k] is the cell used, in [0, src_nt).
 * Returns non-zero (mdq_last_error) and launches nothing when B, S or NP <= 0, when `sparse` lacks its
 * target-mesh arrays, or when only one of srcs / src_of_env is set.
 */
MDQ_API int mdq_interpolate_snapshots(const mdq_interp_desc* d, void* stream);

/* ---- host-side mesh smoothing (DOLFIN Mesh.smooth, flow_solver.py:65-67,236-237) ---- */
/*
 * Gauss-Seidel centroid smoothing of interior vertices in index order, step
 * limited to half the smallest altitude of the vertex star.  Host arrays.
 *   coords [nv][2] in/out; nbr_ptr[nv+1], nbr[]: vertex -> neighbour vertices;
 *   vc_ptr[nv+1], vc[]: vertex -> cell*3+local; cells[nt][3]; on_boundary[nv].
 */
MDQ_API int mdq_smooth_host(double* coords, int32_t nv, const int32_t* cells, int32_t nt,
                    const int64_t* nbr_ptr, const int64_t* nbr, const int64_t* vc_ptr,
                    const int64_t* vc, const uint8_t* on_boundary, int32_t iterations);

/*
 * Batched host mesh engine of the environment step (std::thread over environments):
 * remove one interior vertex per environment (remove_idx[b] < 0: none), restore the Delaunay
 * triangulation of the remaining points by star re-triangulation + Lawson flips (= the reference's
 * global `scipy.spatial.Delaunay` + all-boundary-simplex filter, Env2DAirfoil.py:480-496), then
 * DOLFIN-style smoothing (flow_solver.py:236-237).  Host arrays, in place:
 *   coords [B][NV][2], cells [B][NT][3] (any orientation in; ascending vertex ids per cell out),
 *   nv[B], nt[B] (updated), status[B] (0 ok, <0: star/ear-clipping/flip failure, mesh unusable).
 */
MDQ_API int mdq_remesh_host(int32_t B, int32_t NV, int32_t NT, double* coords, int32_t* cells, int32_t* nv,
                    int32_t* nt, const int32_t* remove_idx, int32_t smooth_iters, int32_t nthreads,
                    int32_t* status);

/*
 * Node features of the state graphs of B environments (Env2DAirfoil.get_state, Env2DAirfoil.py:282-290), including the
 * reference's two indexing quirks (features indexed by n_closest = rank in the removable list; velocity block = raw
 * reshape of the (S,N,2) array).  coords [B][NV][2], u [B][S][NP][2], p [B][S][NV] (f64), n_closest [B][N], nsel [B]
 * (rows >= nsel are zero) -> x [B][N][2+3S] (f32).  All device pointers.
 */
MDQ_API int mdq_state_features(int32_t B, int32_t N, int32_t S, int32_t NV, int32_t NP, const double* coords, const double* u,
                       const double* p, const int32_t* n_closest, const int32_t* nsel, float* x, void* stream);

/*
 * Edge lists of the state graphs (Env2DAirfoil.get_state, Env2DAirfoil.py:258-280) from the padded per-environment
 * arrays of mdq_env_topology to the packed form mdq_gcn_forward reads: the first edge_ptr[b+1] - edge_ptr[b]
 * entries of src_pad / dst_pad [B][EMAX] go to esrc / edst [edge_ptr[b] ...).  All device pointers.
 */
MDQ_API int mdq_compact_edges(int32_t B, int32_t EMAX, const int32_t* src_pad, const int32_t* dst_pad, const int32_t* edge_ptr,
                      int32_t* esrc, int32_t* edst, void* stream);

/* ---- control logic of the batched env step on the device (Env2DAirfoil.step, Env2DAirfoil.py:318-377; calculate_reward
 *      :380-428): with these entry points a rollout is one uninterrupted stream of launches - no read-back between the
 *      Q-network forward and the next vertex removal.  All array arguments are device pointers over B environments. ---- */

/*
 * Action selection + decoding.  q [B][N+1] (or NULL: `action` holds the actions already): the greedy action is the first
 * maximum of a row (torch.argmax, airfoil_dqn.py:208-209); environment b takes rand_action[b] instead where explore[b]
 * (the host draws both arrays from its own random streams ahead of time).  Decoding as in Env2DAirfoil.step: action N
 * shifts the N-closest window (offset[b] += 1), an action without a vertex behind it (>= nsel[b]) gives code 2, otherwise
 * rem[b] = coord_map[b][action] (else -1).  Outputs: action, rem, code [B].
 */
MDQ_API int mdq_env_act(int32_t B, int32_t N, const float* q, const uint8_t* explore, const int32_t* rand_action,
                const int32_t* nsel, const int32_t* coord_map, int32_t* offset, int32_t* action, int32_t* rem,
                int32_t* code, void* stream);

/* its[b] = iterations where a vertex was removed (rem >= 0) and the re-triangulation succeeded (rstat == 0), else 0:
 * the smoothing request of flow_solver.py:236-237 for mdq_smooth. */
MDQ_API int mdq_env_smooth_iters(int32_t B, const int32_t* rem, const int32_t* rstat, int32_t iterations, int32_t* its,
                         void* stream);

/*
 * Reward and terminal flag (Env2DAirfoil.calculate_reward, Env2DAirfoil.py:380-428, + the bookkeeping of step()):
 * new_drags [B][S] (interpolated snapshots' drags on the current mesh), gt_drag [S]; drag reward
 * 2 exp(-(2 ln 2 / threshold) |rel. error|_2) - 1 + time_reward (nv0 - nv); terminal when any relative drag error exceeds
 * the threshold, nv < goal_vertices nv0, the step count reaches `timesteps`, or the step failed (code 2: rstat != 0,
 * nsel < N, topology status != 0 - the latter also sets bit 0 of *err_flag); failed steps get negative_reward.
 * code / steps [B] in/out (steps restart at 0 for terminated environments when auto_reset); reward f64 [B], done u8 [B].
 */
MDQ_API int mdq_env_result(int32_t B, int32_t N, int32_t S, const double* new_drags, const double* gt_drag, const int32_t* nv,
                   int32_t nv0, const int32_t* rstat, const int32_t* topo_status, const int32_t* nsel, int32_t* code,
                   int32_t* steps, double threshold, double time_reward, double goal_vertices, int32_t timesteps,
                   double negative_reward, int32_t auto_reset, double* reward, uint8_t* done, int32_t* err_flag,
                   int32_t* nv_out /* optional [B]: copy of nv (the vertex counts of this step) */, void* stream);

/*
 * mdq_env_result with the LIFT in the reward and in the accuracy stop (appended within ABI 8; not in the reference, whose
 * calculate_reward fills new_lifts and ignores them), and the reason of the stop.  With gl_s = gt_lift[s], nl_s =
 * new_lifts[b][s], w = lift_weight, T = lift_threshold, F = lift_floor, all in fp64, in this order, uncontracted:
 *     el_s        = |gl_s - nl_s| / fmax(|gl_s|, F)            (F: airfoils whose lift passes near zero)
 *     sl          = sum_s el_s^2 (s ascending),  accl = any_s (el_s > T)
 *     lift_reward = 2 exp(-(2 ln 2 / T) sqrt(sl)) - 1
 *     reward (code 0) = (drag_reward + w lift_reward) / (1 + w) + time_reward,    done (code 0) = acc || accl || vert
 * Everything else - drag_reward, time_reward, acc, vert, codes 1 and 2, the step limit - is mdq_env_result's.  The reward stays in
 * [-1, 1] + the time term; a NaN lift gives a NaN reward, as a NaN drag does.  new_lifts [B][S] and gt_lift [S] are both set or
 * both NULL; NULL: the three numbers are not read and every output has the bits of mdq_env_result (which IS this call with
 * NULL lifts and NULL reason); w = 0, T = +inf with finite lifts gives those bits too.  Refused before the launch: one of the
 * two arrays alone; with lifts, w negative / not finite, T not > 0 (+inf is allowed), F negative / not finite.
 * reason [B] (optional, with or without lifts): the bitmask of what ended the step - 1 drag accuracy (acc), 2 lift accuracy
 * (accl), 4 vertex goal (vert), these three for code 0 only; 8 failed step (code neither 0 nor 1); 16 step limit reached (any
 * code) - so that done[b] == (reason[b] != 0).
 */
MDQ_API int mdq_env_result_forces(int32_t B, int32_t N, int32_t S, const double* new_drags, const double* gt_drag,
                   const int32_t* nv, int32_t nv0, const int32_t* rstat, const int32_t* topo_status, const int32_t* nsel,
                   int32_t* code, int32_t* steps, double threshold, double time_reward, double goal_vertices, int32_t timesteps,
                   double negative_reward, int32_t auto_reset, double* reward, uint8_t* done, int32_t* err_flag, int32_t* nv_out,
                   const double* new_lifts /* [B][S] */, const double* gt_lift /* [S] */, double lift_weight,
                   double lift_threshold, double lift_floor, int32_t* reason /* [B] or NULL */, void* stream);

/*
 * Shape quality of the cells of B meshes (appended within ABI 8; not in the reference, which never measures its meshes): one
 * launch, one 256-thread workgroup per environment, no atomics, no scratch, LDS independent of the mesh size.  For a cell with
 * the vertices i0, i1, i2 and the points P0, P1, P2, everything in fp64 and every product, sum and quotient rounded on its own
 * (uncontracted; no sqrt, no transcendental):
 *     ax = x1-x0, ay = y1-y0;  bx = x2-x0, by = y2-y0;  cx = x2-x1, cy = y2-y1
 *     A2 = fabs((ax*by) - (ay*bx))                                      twice the area
 *     s  = ((ax*ax + ay*ay) + (bx*bx + by*by)) + (cx*cx + cy*cy)
 *     q  = s > 0 ? (K * A2) / s : 0       K = 2 sqrt(3) = 3.4641016151377544: 1 equilateral, 0 degenerate
 *     d0 = ax*bx + ay*by;  d1 = -(ax*cx + ay*cy);  d2 = bx*cx + by*cy   dots at the three corners
 *     cot = A2 > 0 ? fmax(d0, fmax(d1, d2)) / A2 : +inf                 cotangent of the cell's smallest angle
 * A cell whose q or cot is not finite, or one of whose vertex ids lies outside [0, nv[b]) (its coordinates are then never
 * loaded), counts as the worst: q = 0, cot = +inf.  Per environment b over the cells [0, nt[b]) (nv[b] / nt[b] are capped at
 * NV / NT): qual[b] = {q_min, cot_max}, the smallest q and the largest cot; qinfo[b] = {cell_q, cell_cot, n_low, 0}, the
 * lowest cell index that attains q_min, the lowest that attains cot_max, and the number of cells with q < q_floor.
 * nt[b] <= 0: {0, +inf} and {-1, -1, 0, 0}.  The results do not depend on the order in which the cells are visited.
 * coords, qual and qinfo must be 16-byte aligned.  Refused before the launch: B, NV or NT <= 0, a NULL pointer, an array not
 * aligned, q_floor not finite or outside [0, 1].
 */
MDQ_API int mdq_mesh_quality(int32_t B, int32_t NV, int32_t NT, const double* coords /* [B][NV][2] */,
                   const int32_t* cells /* [B][NT][3] */, const int32_t* nv, const int32_t* nt, double q_floor,
                   double* qual /* [B][2]: q_min, cot_max */, int32_t* qinfo /* [B][4]: cell_q, cell_cot, n_low, 0 */,
                   void* stream);

/*
 * mdq_env_result_forces with the MESH QUALITY in the reward and as a stop (appended within ABI 8).  With q_min =
 * quality[b][0], cot_max = quality[b][1] (as mdq_mesh_quality writes them), q_ref = quality_ref[0] (device: the q_min of the
 * initial mesh), wq = quality_weight, Qm = min_quality, and max_cot = 1 / tan(min angle), a code-0 step becomes, in fp64, in
 * this order, uncontracted:
 *     quality_reward = 2 fmin(q_min / q_ref, 1) - 1
 *     accq           = (q_min < Qm) || (cot_max > max_cot)
 *     num = drag_reward;  den = 1
 *     lifts set:    num = num + w  * lift_reward;     den = den + w
 *     quality set:  num = num + wq * quality_reward;  den = den + wq
 *     reward = num / den + time_reward,    done = acc || accl || accq || vert,    reason |= 32 where accq
 * quality [B][2] and quality_ref [1] are both set or both NULL; NULL: the three numbers are not read and every output has the
 * bits of mdq_env_result_forces (which IS this call with NULL quality); wq = 0, Qm = 0, max_cot = +inf with a finite quality
 * gives those bits too.  Refused before the launch: one of the two arrays alone; with quality, wq negative / not finite, Qm
 * outside [0, 1), max_cot NaN or <= 0 (+inf, no angle stop, is allowed).
 */
MDQ_API int mdq_env_result_quality(int32_t B, int32_t N, int32_t S, const double* new_drags, const double* gt_drag,
                   const int32_t* nv, int32_t nv0, const int32_t* rstat, const int32_t* topo_status, const int32_t* nsel,
                   int32_t* code, int32_t* steps, double threshold, double time_reward, double goal_vertices, int32_t timesteps,
                   double negative_reward, int32_t auto_reset, double* reward, uint8_t* done, int32_t* err_flag, int32_t* nv_out,
                   const double* new_lifts, const double* gt_lift, double lift_weight, double lift_threshold, double lift_floor,
                   int32_t* reason, const double* quality /* [B][2] */, const double* quality_ref /* [1] */,
                   double quality_weight, double min_quality, double max_cot, void* stream);

/* mdq_restore_rows for the environments with mask[b] != 0 (device array): the in-place reset without a host-side list. */
MDQ_API int mdq_restore_rows_masked(int32_t n, void* const* dst, const void* const* src, const int64_t* row_bytes, int32_t B,
                            const uint8_t* mask, void* stream);

/*
 * The END of a device-resident env step in ONE launch (round 4; before: mdq_copy_strided + mdq_env_result +
 * mdq_restore_rows_masked + mdq_state_features, four launches of 5-9 us each on the latency chain of the step), one
 * environment per workgroup row:
 *   1. reward / terminal flag / codes / step counters exactly as mdq_env_result (Env2DAirfoil.py:380-428, :342-377; with
 *      new_lifts set: as mdq_env_result_forces); the step counters and codes are read from *_in and written to *_out
 *      (several workgroups of an environment read them);
 *   2. every row array t < n_rows (dst[t] laid out [B][row_bytes[t]]): the part [handover_off, + handover_bytes) of
 *      environment b's row is first copied to handover_dst[t] ([B][handover_bytes[t]]; NULL: none) - the meshes and warm-start
 *      fields the flow stream's IPCS leg of THIS step works on, taken before a reset rewrites them - and then, where the
 *      environment terminated and auto_reset is set, the row is overwritten with the cached initial row src[t] (NULL: the
 *      array is handed over only) - Env2DAirfoil.reset, Env2DAirfoil.py:102-129, in place;
 *   3. the node features of the NEXT state (mdq_state_features, Env2DAirfoil.get_state :244-290): computed from the
 *      environment's current arrays, or - for an environment that was just reset - the cached features x_init [N][2 + 3 S]
 *      of the initial state.
 * All pointers are device pointers; sizes / offsets are multiples of 4 bytes (16-byte aligned rows are copied 16 bytes
 * per lane).
 */
#define MDQ_FINISH_MAX_ROWS 16
typedef struct {
  int32_t B, N, S, NV, NP, n_rows;
  int32_t nv0, timesteps, auto_reset, _pad;
  double threshold, time_reward, goal_vertices, negative_reward;
  /* 1. result */
  const double* new_drags;     /* [B][S] */
  const double* gt_drag;       /* [S] */
  const int32_t* nv;           /* [B] */
  const int32_t* rstat;        /* [B] status of mdq_remesh */
  const int32_t* topo_status;  /* [B] status of mdq_env_topology (or NULL) */
  const int32_t* nsel;         /* [B] */
  const int32_t* code_in;      /* [B] codes of the action decoding (mdq_env_act / mdq_remesh_act) */
  int32_t* code_out;           /* [B] */
  const int32_t* steps_in;     /* [B] */
  int32_t* steps_out;          /* [B] (a different array) */
  double* reward;              /* [B] */
  uint8_t* done;               /* [B] */
  int32_t* err_flag;           /* [1] */
  int32_t* nv_out;             /* [B] or NULL */
  /* 2. hand-over + in-place reset */
  void* dst[MDQ_FINISH_MAX_ROWS];
  const void* src[MDQ_FINISH_MAX_ROWS];
  int64_t row_bytes[MDQ_FINISH_MAX_ROWS];
  void* handover_dst[MDQ_FINISH_MAX_ROWS];
  int64_t handover_off[MDQ_FINISH_MAX_ROWS];
  int64_t handover_bytes[MDQ_FINISH_MAX_ROWS];
  /* 3. features of the next state */
  const double* coords;        /* [B][NV][2] (one of the row arrays above) */
  const double* u;             /* [B][S][NP][2] */
  const double* p;             /* [B][S][NV] */
  const int32_t* n_closest;    /* [B][N] */
  const float* x_init;         /* [N][2 + 3 S] or NULL (then auto_reset environments get their features computed too - from
                                  the rows this launch has just restored: only valid with ONE workgroup per environment) */
  float* x;                    /* [B][N][2 + 3 S] */
  int32_t* arrive;             /* [B] arrival counters of the workgroups of an environment, ZERO before the first launch and
                                  left at zero by every launch: the rows among dst[] that ARE nv / nsel - inputs of the
                                  terminal decision every workgroup of the environment takes - are restored by the last
                                  workgroup to have read them.  NULL: one workgroup per environment */
  /* optional (ABI 8), a batch over several airfoils: src_of_env (device [B]) = the airfoil a of environment b.  Set, it
   * switches the fields of the one shared source to per-airfoil tables: gt_drag is [A][S], x_init [A][N][2 + 3 S],
   * nv0_of (device [A], required) replaces nv0, and the cached initial row of row array t for environment b is
   * src[t] + a * src_stride[t] bytes (0: one row shared by every airfoil).  NULL: everything as above. */
  const int32_t* src_of_env;
  const int32_t* nv0_of;
  int64_t src_stride[MDQ_FINISH_MAX_ROWS];
  /* optional (appended within ABI 8), the lift in the reward and in the accuracy stop, exactly as mdq_env_result_forces:
   * new_lifts [B][S] and gt_lift ([S]; with src_of_env [A][S], the row of the environment's airfoil, like gt_drag) are both
   * set or both NULL (then the three numbers are not read: a zero-initialised tail is the drag-only step); a stop on the
   * lift alone resets the environment in place like any other.  reason [B] or NULL: the bitmask of what ended the step. */
  const double* new_lifts;
  const double* gt_lift;
  double lift_weight, lift_threshold, lift_floor;
  int32_t* reason;
  /* optional (appended within ABI 8), the mesh quality in the reward and as a stop, exactly as mdq_env_result_quality:
   * quality [B][2] (q_min, cot_max as mdq_mesh_quality writes them) and quality_ref ([1]; with src_of_env [A], the value of
   * the environment's airfoil) are both set or both NULL (then the three numbers are not read: a zero-initialised tail is
   * the step without the quality part); a stop on the quality alone resets the environment in place like any other. */
  const double* quality;
  const double* quality_ref;
  double quality_weight, min_quality, max_cot;
} mdq_env_finish_desc;
MDQ_API int mdq_env_finish(const mdq_env_finish_desc* d, void* stream);

/*
 * mdq_env_act + mdq_remesh in one launch (the action decoding is the head of the removal kernel; same outputs as the two
 * entry points called one after the other): q / explore / rand_action / nsel / coord_map / offset / action / rem / code as
 * for mdq_env_act, the mesh arguments and status as for mdq_remesh.
 */
MDQ_API int mdq_remesh_act(int32_t B, int32_t NV, int32_t NT, double* coords, int32_t* cells, int32_t* nv, int32_t* nt, int32_t N,
                   const float* q, const uint8_t* explore, const int32_t* rand_action, const int32_t* nsel,
                   const int32_t* coord_map, int32_t* offset, int32_t* action, int32_t* rem, int32_t* code, int32_t* status,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* edge_ptr [B+1] = exclusive prefix sums of nedges [B] (offsets of mdq_compact_edges / mdq_gcn_forward). */
MDQ_API int mdq_edge_ptr(int32_t B, const int32_t* nedges, int32_t* edge_ptr, void* stream);

/*
 * Env2DAirfoil.reset (Env2DAirfoil.py:102-129: mesh, snapshots and selection back to the initial ones) for a SUBSET
 * of the batched environments, in one launch: for each of the n (<= 16) device tensors dst[t], laid out [B][row_bytes[t]],
 * row idx[i] (i < n_idx) is overwritten with the cached initial row src[t].  dst / src / row_bytes are host arrays
 * of device pointers / sizes (4-byte aligned multiples of 4 bytes); idx is a device pointer.
 */
MDQ_API int mdq_restore_rows(int32_t n, void* const* dst, const void* const* src, const int64_t* row_bytes, int32_t n_idx,
                     const int32_t* idx, void* stream);

/*
 * ABI 8: mdq_restore_rows / mdq_restore_rows_masked with one cached initial row PER AIRFOIL: row b of dst[t] is
 * overwritten with src[t] + src_of_env[b] * src_stride[t] bytes (src_stride: host array, multiples of 4; 0 = one row shared
 * by every airfoil); src_of_env: device [B] (B = rows of the destination tensors).
 */
MDQ_API int mdq_restore_rows_src(int32_t n, void* const* dst, const void* const* src, const int64_t* src_stride,
                                 const int64_t* row_bytes, int32_t n_idx, const int32_t* idx, const int32_t* src_of_env,
                                 void* stream);
MDQ_API int mdq_restore_rows_masked_src(int32_t n, void* const* dst, const void* const* src, const int64_t* src_stride,
                                        const int64_t* row_bytes, int32_t B, const uint8_t* mask, const int32_t* src_of_env,
                                        void* stream);

/*
 * DOLFIN `Mesh.smooth(n)` (flow_solver.py:65-67 and 236-237 after every remesh) for B meshes on the GPU: Gauss-Seidel
 * over the interior vertices in index order, each moved towards the centroid of its neighbours by at most half the
 * minimum altitude of its cells; boundary vertices (an incident edge with one owner) are fixed.  One workgroup per
 * mesh: a list schedule of the sweep's dependency graph, walked by one wave out of LDS (exact sequential semantics).  coords [B][NV][2] (in/out),
 * cells [B][NT][3], nv / nt [B], iterations [B] (0 = leave that mesh alone); all device pointers.
 * Capacity: NV <= 1024, NT <= 2048 out of LDS (workspace NULL / 0); up to NV <= 4096, NT <= 8192 through the level-scheduled
 * large-mesh kernel, whose tables live in `workspace` (device, 16-byte aligned, >= mdq_smooth_workspace_bytes(B, NV, NT));
 * up to NV <= 16384, NT <= 32768 (round 6) with the positions in `workspace` as well (-1 beyond that).
 */
MDQ_API int64_t mdq_smooth_workspace_bytes(int32_t B, int32_t NV, int32_t NT);
MDQ_API int mdq_smooth(int32_t B, int32_t NV, int32_t NT, double* coords, const int32_t* cells, const int32_t* nv,
               const int32_t* nt, const int32_t* iterations, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The same smoothing, faster: a Gauss-Seidel sweep in which every vertex takes the full step is the linear system
 * (D - L) x_new = U x_old: the sweeps run as blocked triangular solves (32-row blocks, inverses built once per launch),
 * every sweep is validated in parallel (was each update clearly a full step?), and a sweep that was not is redone from
 * its snapshot with the offending vertices on DOLFIN's exact (limited-step) update and a rank-1 correction of their block:
 * exact sequential semantics, results equal to mdq_smooth to round-off (different association).  A mesh beyond the
 * kernel's limits (more than 16 cells at a vertex) is handed to mdq_smooth's kernel.  Same arguments as mdq_smooth + a
 * device workspace of at least mdq_smooth_fast_workspace_bytes(B, NV) bytes, 16-byte aligned (block inverses,
 * per-environment diagnostics).
 */
MDQ_API int64_t mdq_smooth_fast_workspace_bytes(int32_t B, int32_t NV);
MDQ_API int mdq_smooth_fast(int32_t B, int32_t NV, int32_t NT, double* coords, const int32_t* cells, const int32_t* nv,
                    const int32_t* nt, const int32_t* iterations, void* workspace, int64_t workspace_bytes, void* stream);
/* Inside an env step (Env2DAirfoil._check_mesh -> flow_solver.remesh -> smooth(50), flow_solver.py:236-237): `iterations`
 * sweeps for the environments whose vertex removal succeeded (rem[b] >= 0 and rstat[b] == 0, the outputs of mdq_env_act /
 * mdq_remesh), none for the others - mdq_env_smooth_iters + mdq_smooth_fast in one launch. */
MDQ_API int mdq_smooth_fast_env(int32_t B, int32_t NV, int32_t NT, double* coords, const int32_t* cells, const int32_t* nv,
                        const int32_t* nt, const int32_t* rem, const int32_t* rstat, int32_t iterations, void* workspace,
                        int64_t workspace_bytes, void* stream);

/*
 * Diagnostics of mdq_smooth since the last reset (no reference counterpart): out64[s], s < 63 = speculative sweeps s
 * that met an update that was not clearly a full step and were redone by careful sweeps (see mdq_smooth.hip).
 * out64 is a HOST array of 64 int64 (may be NULL); reset != 0 zeroes the counters.  Synchronises the device.
 */
MDQ_API int mdq_smooth_stats(int64_t* out64, int32_t reset);

/*
 * Env2DAirfoil._remove_vertex (Env2DAirfoil.py:452-512) for B meshes on the GPU, WITHOUT the smoothing (mdq_smooth):
 * ear clipping of the removed vertex's star polygon + Lawson flips to the (unique) Delaunay triangulation = the
 * reference's global scipy Delaunay + all-boundary filter as a set of cells; vertex ids above the removed one shift
 * down; cells are written with ascending vertex ids.  remove_idx[b] < 0 leaves mesh b untouched.  status[b]: 0 ok,
 * -1..-4 star / boundary vertex / ear clipping failures, -11 non-manifold, -12 flip work list exhausted (mesh b is
 * untouched on failure).  All pointers are device pointers.  Capacity: NV <= 1024, NT <= 2048 with every table in LDS
 * (workspace NULL / 0); up to NV <= 4096, NT <= 8192 with the tables in `workspace` (device, 16-byte aligned, at least
 * mdq_remesh_workspace_bytes(B, NV, NT) bytes: 0 for the LDS instance, -1 beyond the kernels) and the edge hash in LDS; up to
 * NV <= 16384, NT <= 32768 (round 6) with the edge hash in `workspace` as well.
 */
MDQ_API int64_t mdq_remesh_workspace_bytes(int32_t B, int32_t NV, int32_t NT);
MDQ_API int mdq_remesh(int32_t B, int32_t NV, int32_t NT, double* coords, int32_t* cells, int32_t* nv, int32_t* nt,
               const int32_t* remove_idx, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- optional outputs of mdq_env_topology_host: the index data of the matrix-free IPCS path (mode 3 with the CG
 *      pressure solver) on every coarsened mesh, i.e. what FlowSolver.__init__/remesh derive from the mesh
 *      (flow_solver.py:85-132,194-226) minus the assembled patterns.  Same layouts as the mdq_ipcs_desc fields of the
 *      same names; feed them (uploaded) to mdq_ipcs_setup_matfree + mdq_ipcs_evolve. ---- */
typedef struct mdq_ipcs_topo_out {
  int32_t NBO, NBE, NSE1;  /* capacities: outflow rows, outflow entries, SELL-64 entries of the P1 Laplacian */
  int32_t flow_only;      /* mdq_env_topology: != 0 skips `removable`, the polygon distances / N-closest window and the state
                             graph (nremovable / nsel / n_closest / coord_map / nedges / edge_* are left untouched): the run of
                             an engine that only feeds the IPCS step (the flow stream of the S3 env step) */
  int32_t* mf_scat;       /* [B][6][NT]  dof | (outflow_edge+1) << 28 (word 0) */
  int8_t* cell_outflow;   /* [B][NT]     local outflow facet or -1 */
  uint8_t* bcu_flag;      /* [B][NP] */
  double* bcu_gx;         /* [B][NP] */
  uint8_t* bcp_flag;      /* [B][NV] */
  int32_t* nbo;           /* [B] */
  int32_t* bo_rows;       /* [B][NBO] */
  int32_t* bo_ptr;        /* [B][NBO+1] */
  int32_t* bo_col;        /* [B][NBE] */
  int32_t* bo_src;        /* [B][NBE] */
  int32_t* g1_ptr;        /* [B][NV+1] */
  int32_t* g1_src;        /* [B][3*NT] */
  int32_t* g2_ptr;        /* [B][NP+1] */
  int32_t* g2_src;        /* [B][6*NT] */
  int32_t* sl1_off;       /* [B][NV/64+2] */
  int32_t* sl1_col;       /* [B][NSE1] */
  /* optional inputs of a `flow_only` run of mdq_env_topology (both NULL: the edges are numbered here): the cell dofs
   * [B][6][NT] and edge counts [B] that another engine's run derived from the SAME meshes - the edge numbering is taken
   * from them instead of being found again through the hash table */
  const int32_t* cell_dofs_in;
  const int32_t* ne_in;
} mdq_ipcs_topo_out;

/* ---- batched topology + N-closest selection + state graph (host arrays) ---- */
/* Optional second set of outputs of mdq_env_topology (device engine only; ABI 5, round 4): copies of the mesh and of its
 * edge numbering for ANOTHER engine that works on the same meshes on another stream - the flow leg of the S3 env step
 * (VecEnv2DAirfoil, flow_overlap): written by the topology kernel itself, so that the other stream can start as soon as this
 * launch has finished instead of waiting for a copy launch behind it.  A HOST struct holding device pointers. */
typedef struct mdq_topo_handover {
  double* coords;           /* [B][NV][2] rows < nv */
  int32_t* cells;           /* [B][NT][3] rows < nt */
  int32_t* nv;              /* [B] */
  int32_t* nt;              /* [B] */
  int32_t* cell_dofs;       /* [B][6][NT] */
  int32_t* ne;              /* [B] */
} mdq_topo_handover;

typedef struct mdq_env_topo_desc {
  int32_t B, NV, NT, NP, NAF, N, EMAX, npoly;   /* capacities; N = N_closest; npoly = airfoil polygon points */
  /* inputs */
  const double* coords;     /* [B][NV][2] */
  const int32_t* cells;     /* [B][NT][3]  ascending vertex ids per cell */
  const int32_t* nv;        /* [B] */
  const int32_t* nt;        /* [B] */
  const int32_t* offset;    /* [B]  do_nothing_offset (Env2DAirfoil.py:308) */
  const double* polygon;    /* [npoly][2]  airfoil boundary points of the ORIGINAL mesh in vertex order (:223-233) */
  /* outputs */
  int32_t* ne;              /* [B] */
  int32_t* cell_dofs;       /* [B][6][NT]  P2 dofs (edges numbered by first appearance) */
  double* points;           /* [B][NP][2]  P2 dof coordinates: vertices, then edge midpoints */
  int32_t* naf;             /* [B] */
  int32_t* af_facets;       /* [B][NAF][2] (cell, local edge) of the airfoil facets */
  int32_t* nremovable;      /* [B] */
  int32_t* nsel;            /* [B]  min(N, removable - offset) */
  int32_t* n_closest;       /* [B][N]  ranks inside the removable list (the reference indexes features with these) */
  int32_t* coord_map;       /* [B][N]  vertex id of every action */
  int32_t* nedges;          /* [B] */
  int32_t* edge_src;        /* [B][EMAX] */
  int32_t* edge_dst;        /* [B][EMAX] */
  double* edge_len;         /* [B][EMAX] edge_attr */
  const mdq_ipcs_topo_out* ipcs;  /* optional (NULL: skip) */
  const mdq_topo_handover* handover;  /* optional (NULL: none; ignored by the host engine) */
  void* workspace;          /* device, 16-byte aligned, >= mdq_env_topology_workspace_bytes(d) bytes: the tables of the
                               large-mesh kernel instance (NULL / 0 for meshes of up to 1024 vertices and for the host engine) */
  int64_t workspace_bytes;
  /* optional (ABI 8), a batch over several airfoils: `polygon` holds the A polygons one after the other, poly_ptr [A+1]
   * their first points, src_of_env [B] the airfoil of every environment (environment b measures its distances to points
   * poly_ptr[a] .. poly_ptr[a+1] - 1, a = src_of_env[b]); npoly is then the largest of the A polygons.  Both NULL: the one
   * polygon [npoly][2].  Device pointers for mdq_env_topology, host pointers for mdq_env_topology_host. */
  const int32_t* poly_ptr;
  const int32_t* src_of_env;
} mdq_env_topo_desc;

/*
 * Per environment: unique edges / P2 dof map / dof coordinates, boundary + airfoil facets, `removable`
 * (flow_solver.py:75-78 quirk), polygon distances + argsort + N-closest window (Env2DAirfoil.py:220-241,
 * 293-315) and the state graph edges (:258-280).  status[b] = 0 ok, <0 capacity exceeded
 * (-1 NP, -2 NAF, -3 EMAX, -4 more than 2 outflow rows per row-owner thread, -5 NBO/NBE, -6 NSE1, -7 the environment's
 * polygon (poly_ptr) is empty or larger than npoly).
 */
MDQ_API int mdq_env_topology_host(const mdq_env_topo_desc* d, int32_t nthreads, int32_t* status);

/*
 * The same engine as a HIP kernel (one workgroup per environment, everything in LDS): every pointer of the descriptor
 * (and of d->ipcs, a HOST struct holding device pointers) and `status` are DEVICE pointers.  All output arrays are
 * bit-identical to mdq_env_topology_host's.  Capacity: NV <= 1024, NT <= 2048, NP <= 4096 with every table in LDS; up to
 * NV <= 4096, NT <= 8192, NP <= 16384 with the tables in d->workspace (mdq_env_topology_workspace_bytes: 0 for the LDS
 * instance, -1 beyond the kernels), npoly <= 256; up to NV <= 16384, NT <= 32768, NP <= 65536 (round 6: every table incl.
 * the edge hash and the coordinates in d->workspace), npoly <= 512.
 */
MDQ_API int64_t mdq_env_topology_workspace_bytes(const mdq_env_topo_desc* d);
MDQ_API int mdq_env_topology(const mdq_env_topo_desc* d, void* stream, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* MESHDQN_HIP_H */
