// IPCS, shared: element right-hand sides, the matrix-free operator applications (LDS tiles, global tiles of mode 5), the
// workgroup-wide SELL kernels and the Krylov solvers with cg_pressure.  Included by all four IPCS units, behind the views.
namespace mdq {

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
                                            const double2 (&xe)[6], double2 (&ye)[6]) {
  elem_velocity(g, a, mu, xe, ye);
  if (ko >= 0) {
    double X[3][2];
    load_cell_coords(v, e, X);
    elem_outflow_add(g, X, ko, -0.5 * mu, xe, ye);
  }
}

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

}  // namespace mdq
