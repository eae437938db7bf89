// IPCS: non-separable inflow profiles (inflow_lift_kernel, launch_inflow_lift) and the inlet map of a device-built mesh.
// Included by mdq_ipcs.hip (the entry unit) only, behind the reference tables.
namespace mdq {

// ================================================================== inflow profile (mdq_ipcs_evolve_profile)
//
// The inflow of ONE step of a launch sequence: values[b][step] scattered into bcu_gx at the inlet dofs, then lift1 / lift3
// recomputed on the rows that share a cell with an inlet dof - the three things of the set-up that depend on the Dirichlet
// vector (the elimination is linear in it and only the inlet is non-zero).  The per-row sums are the "P2 rows" loop of
// setup_matfree_kernel restated (not shared: that kernel's resource row stays what it is): slots through g2_ptr / g2_src,
// the cell's geom and cell_dofs, every flagged column j adds bx gx, bz gx, m gx.  A row list is a few dozen rows of ~6 cells, each
// cell a chain of four dependent loads, so a row is spread over 8 lanes (one slot each) and summed by a fixed shuffle tree:
// one pass of the workgroup for up to 64 rows, the order fixed, no atomics.  Outflow rows are not in the list (the host
// refuses such a mesh): their - mu/2 B correction is not re-applied.  Writes bcu_gx[inlet], lift1[rows], lift3[rows] only.
constexpr int IWG = 512;   // 64 rows x 8 lanes per pass
static __global__ __launch_bounds__(IWG) void inflow_lift_kernel(mdq_ipcs_desc d, mdq_inflow_profile pr, int nsteps, int step) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const EnvView v = env_view(d, b);
  const double a = v.rho / v.dt, mu = v.mu;
  __shared__ double sMhat[6][6];
  __shared__ double sGhat[2][2][6][6];
  for (int q = tid; q < 36; q += IWG) sMhat[q / 6][q % 6] = c_tab.Mhat[q / 6][q % 6];
  for (int q = tid; q < 144; q += IWG) sGhat[q / 72][(q / 36) % 2][(q / 6) % 6][q % 6] = c_tab.Ghat[q / 72][(q / 36) % 2][(q / 6) % 6][q % 6];
  const int nin = min(pr.n_inlet[b], pr.NIN), nr = min(pr.n_rows[b], pr.NIR);
  const int32_t* dofs = pr.inlet_dofs + (int64_t)b * pr.NIN;
  const double* val = pr.values + ((int64_t)b * nsteps + step) * pr.NIN;
  // (an input of every other entry point, hence const in the descriptor; this one is documented to rewrite its inlet entries)
  double* gxw = const_cast<double*>(d.bcu_gx) + (int64_t)b * d.N2;
  for (int k = tid; k < nin; k += IWG) {
    const int i = dofs[k];
    if (i >= 0 && i < v.n2) gxw[i] = val[k];
  }
  __syncthreads();   // (the new Dirichlet values and the tables are visible to the workgroup)
  const int32_t* rows = pr.rows + (int64_t)b * pr.NIR;
  const int sub = tid & 7;
  for (int base = 0; base < nr; base += IWG / 8) {   // (uniform trip count: every lane takes part in the shuffles)
    const int q = base + (tid >> 3);
    const int r = q < nr ? rows[q] : -1;
    const bool ok = r >= 0 && r < v.n2;
    double l1x = 0.0, l1y = 0.0, l3x = 0.0;
    if (ok) {
      const int s1 = v.g2_ptr[r + 1];
      for (int s = v.g2_ptr[r] + sub; s < s1; s += 8) {
        const int slot = v.g2_src[s];
        const int e = slot / 6, i = slot - e * 6;
        const Geo g = load_geo(v, e);
        int cj[6];
        bool fj[6];
        double gj[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) cj[j] = v.cell_dofs[j * v.NT + e];
#pragma unroll
        for (int j = 0; j < 6; ++j) fj[j] = v.bcu_flag[cj[j]] != 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) gj[j] = fj[j] ? gxw[cj[j]] : 0.0;
        const double Ja[2][2] = {{g.j00, g.j01}, {g.j10, g.j11}};
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          if (!fj[j]) continue;
          const double m = g.det * sMhat[i][j];
          const double g00 = sGhat[0][0][i][j], g01 = sGhat[0][1][i][j];
          const double g10 = sGhat[1][0][i][j], g11 = sGhat[1][1][i][j];
          const double kxx = g.det * (Ja[0][0] * (Ja[0][0] * g00 + Ja[1][0] * g01) + Ja[1][0] * (Ja[0][0] * g10 + Ja[1][0] * g11));
          const double kxy = g.det * (Ja[0][0] * (Ja[0][1] * g00 + Ja[1][1] * g01) + Ja[1][0] * (Ja[0][1] * g10 + Ja[1][1] * g11));
          const double kyy = g.det * (Ja[0][1] * (Ja[0][1] * g00 + Ja[1][1] * g01) + Ja[1][1] * (Ja[0][1] * g10 + Ja[1][1] * g11));
          const double L = kxx + kyy;
          const double bx = a * m + 0.5 * mu * (L + kxx), bz = 0.5 * mu * kxy;
          l1x += bx * gj[j];
          l1y += bz * gj[j];
          l3x += m * gj[j];
        }
      }
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {
      l1x += __shfl_down(l1x, o, 8);
      l1y += __shfl_down(l1y, o, 8);
      l3x += __shfl_down(l3x, o, 8);
    }
    if (ok && sub == 0) {
      v.lift1[r] = make_double2(l1x, l1y);
      v.lift3[r] = make_double2(l3x, 0.0);
    }
  }
}

// ================================================================== inlet map of a device-built mesh (mdq_ipcs_build_inlet_map)
//
// The tables inflow_lift_kernel reads - inlet dofs and inlet-adjacent rows - for a mesh whose dofs were numbered on the
// device (the S3 flow leg: every step a new mesh).  The inlet POINTS never change (boundary vertices are neither removed nor
// moved, the inlet facets lie on the convex hull), only their numbers: the caller hands over the canonical inlet of the
// ORIGINAL mesh, its y ascending (inlet_y[b][0 .. n_ref[b])), and the kernel finds which dof of this mesh is which point.
// PRECONDITION: bcu_gx holds what the topology run wrote, the constant parabola - non-zero exactly on the inlet dofs the
// airfoil / wall conditions do not override (the two corner vertices sit at y = bot / top: overridden, and the parabola is
// zero there anyway); it runs before any profile step has rewritten bcu_gx.  Reads cell_dofs, coords, nv / nt / ne, bcu_flag,
// bcu_gx, cell_outflow.  One workgroup per environment, one pass over the dofs and two over the cells:
//   inlet set   dof i < n2 with bcu_flag[i] != 0 && bcu_gx[i] != 0: a bitmap over n2 in LDS; its position in the set (the
//               number of set bits below it, from a per-word prefix) is its slot in the LDS lists
//   y           from a cell that holds the dof: a vertex's coords, or 0.5 * (ya + yb) of the edge opposite vertex k for local
//               dof 3 + k - the expression of MeshTopology.dof_coords, so the bits agree (an inlet edge has one cell; the
//               cells of an inlet vertex all store the same bits)
//   order       rank r = the number of inlet dofs with a smaller y (ties - there are none on an inlet - by slot, so the ranks
//               are a permutation whatever the input); inlet_dofs[b][r] = that dof, |y - inlet_y[b][r]| <= 1e-12 (top - bot)
//               with top - bot the extent of the mesh's vertices in y (what the topology run and the host use as H)
//   rows        every dof with bcu_flag == 0 of every cell that holds an inlet dof: a second bitmap (LDS atomicOr: the result
//               does not depend on the order), compacted by the same per-word prefix -> unique, ascending, no global atomics
// map_status[b] (sticky: written only while it is 0) takes the first failure: 1 inlet count != n_ref[b] (or beyond NIN / the
// 64 slots of the LDS lists), 2 a y differs, 3 more rows than NIR, 4 an inlet-adjacent free row is a row of an outflow facet
// (inflow_lift_kernel does not re-apply their correction).  A failing environment gets n_inlet = n_rows = 0 and lists of -1.
// Every index read from the mesh is range-checked and every write stays inside [b][NIN] / [b][NIR] whatever the input.
constexpr int MWG = 256;       // latency-bound: ~6 cells per thread on the lab meshes, 4 waves = one per SIMD
constexpr int MAP_BITS = 3584; // the bitmaps cover the meshes of the LDS-resident modes (MF_ROWS * WG rows)
constexpr int MAP_WORDS = MAP_BITS / 32;
constexpr int MAP_NIN = 64;    // slots of the LDS inlet lists (lab meshes: about a dozen inlet dofs)
static __global__ __launch_bounds__(MWG) void inlet_map_kernel(mdq_ipcs_desc d, int NIN, int NIR, const int32_t* n_ref,
                                                               const double* inlet_y, int32_t* n_inlet, int32_t* inlet_dofs,
                                                               int32_t* n_rows, int32_t* rows, int32_t* map_status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ unsigned s_in[MAP_WORDS], s_row[MAP_WORDS];
  __shared__ int s_pre[MAP_WORDS + 1];
  __shared__ double s_y[MAP_NIN];
  __shared__ int s_dof[MAP_NIN], s_sorted[MAP_NIN];
  __shared__ double s_lo[MWG / 64], s_hi[MWG / 64];
  __shared__ int s_bad_y, s_bad_out;
  const int nv = min(max(d.nv[b], 0), d.NV), nt = min(max(d.nt[b], 0), d.NT), ne = min(max(d.ne[b], 0), d.NE);
  const int n2 = min(nv + ne, MAP_BITS);
  const int64_t B = b;
  const double* coords = d.coords + B * d.NV * 2;
  const int32_t* cd = d.cell_dofs + B * 6 * d.NT;
  const int8_t* cof = d.cell_outflow + B * d.NT;
  const uint8_t* fl = d.bcu_flag + B * d.N2;
  const double* gx = d.bcu_gx + B * d.N2;
  for (int w = tid; w < MAP_WORDS; w += MWG) s_in[w] = s_row[w] = 0u;
  for (int k = tid; k < MAP_NIN; k += MWG) {
    s_y[k] = 0.0;
    s_dof[k] = s_sorted[k] = -1;
  }
  if (tid == 0) s_bad_y = s_bad_out = 0;
  // extent of the mesh in y (fixed tree: lanes by shuffle, waves through LDS)
  double lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < nv; i += MWG) {
    const double y = coords[2 * i + 1];
    lo = fmin(lo, y);
    hi = fmax(hi, y);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, o));
    hi = fmax(hi, __shfl_xor(hi, o));
  }
  if ((tid & 63) == 0) {
    s_lo[tid >> 6] = lo;
    s_hi[tid >> 6] = hi;
  }
  __syncthreads();
  // inlet set
  for (int i = tid; i < n2; i += MWG)
    if (fl[i] != 0 && gx[i] != 0.0) atomicOr(&s_in[i >> 5], 1u << (i & 31));
  __syncthreads();
  auto word_prefix = [&](const unsigned* bits) {   // s_pre[w] = set bits in the words below w; s_pre[MAP_WORDS] = all
    for (int w = tid; w <= MAP_WORDS; w += MWG) {
      int s = 0;
      for (int q = 0; q < w; ++q) s += __popc(bits[q]);
      s_pre[w] = s;
    }
  };
  auto slot_of = [&](const unsigned* bits, int i) { return s_pre[i >> 5] + __popc(bits[i >> 5] & ((1u << (i & 31)) - 1u)); };
  auto has = [&](const unsigned* bits, int i) { return (bits[i >> 5] >> (i & 31)) & 1u; };
  word_prefix(s_in);
  __syncthreads();
  double H = 0.0;
  {
    double l = s_lo[0], h = s_hi[0];
#pragma unroll
    for (int q = 1; q < MWG / 64; ++q) {
      l = fmin(l, s_lo[q]);
      h = fmax(h, s_hi[q]);
    }
    H = h - l;
  }
  const int nin = s_pre[MAP_WORDS], want = n_ref[b];
  int fail = (nin != want || nin > NIN || nin > MAP_NIN) ? 1 : 0;   // (workgroup-uniform from here on)
  if (!fail) {
    // cells: y of the inlet dofs, the rows around them
    for (int e = tid; e < nt; e += MWG) {
      int c[6];
      bool in_range = true;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        c[j] = cd[j * d.NT + e];
        in_range = in_range && c[j] >= 0 && c[j] < n2 && (j >= 3 || c[j] < nv);
      }
      if (!in_range) continue;
      unsigned m = 0;
#pragma unroll
      for (int j = 0; j < 6; ++j) m |= has(s_in, c[j]) << j;
      if (!m) continue;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        if (fl[c[j]] == 0) atomicOr(&s_row[c[j] >> 5], 1u << (c[j] & 31));
        if (!((m >> j) & 1u)) continue;
        double y;
        if (j < 3) {
          y = coords[2 * c[j] + 1];
        } else {
          const int k = j - 3, va = c[k == 0 ? 1 : 0], vb = c[k == 2 ? 1 : 2];
          y = 0.5 * (coords[2 * va + 1] + coords[2 * vb + 1]);
        }
        const int slot = slot_of(s_in, c[j]);   // (< nin <= MAP_NIN)
        s_y[slot] = y;
        s_dof[slot] = c[j];
      }
    }
    __syncthreads();
    // canonical order
    const double tol = 1e-12 * H;
    for (int t = tid; t < nin; t += MWG) {
      const double y = s_y[t];
      int r = 0;
      for (int k = 0; k < nin; ++k) r += (s_y[k] < y || (s_y[k] == y && k < t)) ? 1 : 0;
      s_sorted[r] = s_dof[t];
      if (s_dof[t] < 0 || !(fabs(y - inlet_y[B * NIN + r]) <= tol)) atomicOr(&s_bad_y, 1);
    }
    __syncthreads();
    word_prefix(s_row);
    // a row of an outflow facet among them?
    for (int e = tid; e < nt; e += MWG) {
      const int k = cof[e];
      if (k < 0 || k > 2) continue;
      const int loc[3] = {k == 0 ? 1 : 0, k == 2 ? 1 : 2, 3 + k};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int i = cd[loc[q] * d.NT + e];
        if (i >= 0 && i < n2 && has(s_row, i)) atomicOr(&s_bad_out, 1);
      }
    }
    __syncthreads();
    fail = s_bad_y ? 2 : (s_pre[MAP_WORDS] > NIR ? 3 : (s_bad_out ? 4 : 0));
  }
  const int nr = fail ? 0 : s_pre[MAP_WORDS], nok = fail ? 0 : nin;
  int32_t* od = inlet_dofs + B * NIN;
  int32_t* orow = rows + B * NIR;
  for (int r = tid; r < NIN; r += MWG) od[r] = r < nok ? s_sorted[r] : -1;
  for (int q = nr + tid; q < NIR; q += MWG) orow[q] = -1;
  if (!fail)
    for (int i = tid; i < n2; i += MWG)
      if (has(s_row, i)) orow[slot_of(s_row, i)] = i;   // (slot < nr <= NIR)
  if (tid == 0) {
    n_inlet[b] = nok;
    n_rows[b] = nr;
    if (fail && map_status[b] == 0) map_status[b] = fail;
  }
}

hipError_t launch_inflow_lift(const mdq_ipcs_desc* d, const mdq_inflow_profile* prof, int nsteps, int step, hipStream_t st) {
  hipLaunchKernelGGL(inflow_lift_kernel, dim3(d->B), dim3(IWG), 0, st, *d, *prof, nsteps, step);
  return hipGetLastError();
}

}  // namespace mdq
