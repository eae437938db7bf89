// Mesh-side kernels of the environment step: point location + P2/P1 evaluation of the stored
// snapshots on a coarsened mesh (Env2DAirfoil._check_mesh, Env2DAirfoil.py:556-593:
// `v_func.interpolate(original_u)`, `p_func.interpolate(original_p)` and the vertex evaluations).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "../../include/meshdqn_hip.h"
#include "mdq_internal.h"

namespace mdq_mesh {

// One thread per target point: walk the candidate cells of its grid bin (ascending cell id), take the
// first cell whose barycentric coordinates are all >= 0, otherwise the candidate with the smallest
// violation, then evaluate all snapshots with the P2 / P1 bases of that cell.
// Outside every cell the choice is bin-local: the least violated candidate of the point's bin (beyond the
// far field the bin clamped to the grid's edge; deep in the airfoil an empty bin, which holds only the cell
// with the centroid nearest to its centre), not the mesh's closest cell of DOLFIN's `allow_extrapolation`;
// the values are that cell's polynomials, extrapolated.  The environment never reaches beyond round-off:
// of the P2 dof points of both golden episodes (154 752 and 140 496 points, 48 coarsened meshes each),
// 1.6 % and 1.2 % lie in no cell, all on shared or boundary edges, outside by at most 1.9e-15 in
// barycentric coordinates (tests/test_interp_probe_gpu.py).
__global__ __launch_bounds__(256) void interpolate_kernel(mdq_interp_desc d) {
  const int b = blockIdx.y;
  // the source of this environment (workgroup-uniform): the descriptor's own fields, or - a batch over several airfoils -
  // the record of its airfoil
  mdq_interp_src src;
  if (d.srcs) {
    src = d.srcs[__builtin_amdgcn_readfirstlane(d.src_of_env[b])];
  } else {
    src.src_nv = d.src_nv;
    src.src_nt = d.src_nt;
    src.src_n2 = d.src_n2;
    src.gnx = d.gnx;
    src.gny = d.gny;
    src.x0 = d.x0;
    src.y0 = d.y0;
    src.inv_hx = d.inv_hx;
    src.inv_hy = d.inv_hy;
    src.src_coords = d.src_coords;
    src.src_cell_dofs = d.src_cell_dofs;
    src.src_geom = d.src_geom;
    src.bin_ptr = d.bin_ptr;
    src.bin_cells = d.bin_cells;
    src.src_u = d.src_u;
    src.src_p = d.src_p;
    src.src_cellrec = d.src_cellrec;
  }
  const int npts = d.npts[b] + (d.npts_extra ? d.npts_extra[b] : 0);
  const int np1 = d.np1[b];
  const int64_t B = b;
  const double* pts = d.points + B * d.NP * 2;
  // sparse mode (see the header): blocks [0, nbA) walk the points - vertices every snapshot, edge midpoints the last one
  // (or none) - blocks [nbA, gridDim.x) the three edges of the airfoil-facet cells, the remaining snapshots
  const int nbA = d.sparse ? (d.NP + 255) / 256 : (int)gridDim.x;
  const bool passB = (int)blockIdx.x >= nbA;
  const int nB = passB ? 3 * d.naf[b] : 0;
  const int kfirst = passB ? ((int)blockIdx.x - nbA) * (int)blockDim.x + (int)threadIdx.x : (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int kstride = passB ? ((int)gridDim.x - nbA) * (int)blockDim.x : nbA * (int)blockDim.x;
  for (int kk = kfirst; kk < (passB ? nB : npts); kk += kstride) {
    int k = kk, s_lo = 0, s_hi = d.S;
    if (passB) {
      const int f = kk / 3, j = kk - 3 * f;
      const int cell = d.af_facets[(B * d.NAF + f) * 2];
      k = d.cell_dofs[(B * 6 + 3 + j) * d.NT + cell];
      if (d.sparse == 1) s_hi = d.S - 1;          // (the last snapshot of every edge midpoint is pass A's)
      if (k < np1 || k >= npts || s_hi <= s_lo) continue;
    } else if (d.sparse && k >= np1) {
      if (d.sparse == 2) continue;
      s_lo = d.S - 1;
    }
    const double px = pts[2 * k], py = pts[2 * k + 1];
    int gx = (int)floor((px - src.x0) * src.inv_hx), gy = (int)floor((py - src.y0) * src.inv_hy);
    gx = gx < 0 ? 0 : (gx >= src.gnx ? src.gnx - 1 : gx);
    gy = gy < 0 ? 0 : (gy >= src.gny ? src.gny - 1 : gy);
    const int bin = gy * src.gnx + gx;
    int best = -1;
    double bxi = 0.0, beta = 0.0, bviol = -1e300;
    if (src.src_cellrec) {
      // candidates in batches of CB: their ids in one round trip, their records (vertex 0 + Jinv, 48 bytes) in a second
      // one, then the same tests in the same order.  (Cell by cell - id, then its dofs, then the vertex - a point paid
      // three dependent L2 round trips per candidate: the whole kernel was the latency of its longest candidate list.)
      constexpr int CB = 6;
      const int s0 = src.bin_ptr[bin], s1 = src.bin_ptr[bin + 1];
      bool found = false;
      for (int sb = s0; sb < s1 && !found; sb += CB) {
        int cid[CB];
#pragma unroll
        for (int q = 0; q < CB; ++q) cid[q] = src.bin_cells[min(sb + q, s1 - 1)];
        double2 r0[CB], r1[CB], r2[CB];
#pragma unroll
        for (int q = 0; q < CB; ++q) {
          const double2* rp = reinterpret_cast<const double2*>(src.src_cellrec + (int64_t)cid[q] * 6);
          r0[q] = rp[0];
          r1[q] = rp[1];
          r2[q] = rp[2];
        }
#pragma unroll
        for (int q = 0; q < CB; ++q) {
          if (sb + q < s1 && !found) {
            const double dx = px - r0[q].x, dy = py - r0[q].y;
            const double xi = r1[q].x * dx + r1[q].y * dy, eta = r2[q].x * dx + r2[q].y * dy;
            const double l0 = 1.0 - xi - eta;
            double viol = fmin(fmin(l0, xi), eta);
            viol = viol < 0.0 ? viol : 0.0;
            if (viol > bviol) {  // strict: the first (lowest id) best candidate wins
              bviol = viol;
              best = cid[q];
              bxi = xi;
              beta = eta;
              if (viol == 0.0) found = true;
            }
          }
        }
      }
    } else
    for (int s = src.bin_ptr[bin]; s < src.bin_ptr[bin + 1]; ++s) {
      const int c = src.bin_cells[s];
      const int v0 = src.src_cell_dofs[0 * src.src_nt + c];
      const double dx = px - src.src_coords[2 * v0], dy = py - src.src_coords[2 * v0 + 1];
      const double j00 = src.src_geom[0 * src.src_nt + c], j01 = src.src_geom[1 * src.src_nt + c];
      const double j10 = src.src_geom[2 * src.src_nt + c], j11 = src.src_geom[3 * src.src_nt + c];
      // reference coordinates: [xi, eta] = J^-1 (x - x0); geom stores Jinv[c][a] (reference row, physical col)
      const double xi = j00 * dx + j01 * dy, eta = j10 * dx + j11 * dy;
      const double l0 = 1.0 - xi - eta;
      double viol = fmin(fmin(l0, xi), eta);
      viol = viol < 0.0 ? viol : 0.0;
      if (viol > bviol) {  // strict: the first (lowest id) best candidate wins
        bviol = viol;
        best = c;
        bxi = xi;
        beta = eta;
        if (viol == 0.0) break;
      }
    }
    const double l0 = 1.0 - bxi - beta, l1 = bxi, l2 = beta;
    double phi[6];
    phi[0] = l0 * (2.0 * l0 - 1.0);
    phi[1] = l1 * (2.0 * l1 - 1.0);
    phi[2] = l2 * (2.0 * l2 - 1.0);
    phi[3] = 4.0 * l1 * l2;
    phi[4] = 4.0 * l0 * l2;
    phi[5] = 4.0 * l0 * l1;
    int dof[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) dof[i] = src.src_cell_dofs[i * src.src_nt + best];
    for (int s = s_lo; s < s_hi; ++s) {
      const double* us = src.src_u + (int64_t)s * src.src_n2 * 2;
      double ux = 0.0, uy = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        ux += us[2 * dof[i]] * phi[i];
        uy += us[2 * dof[i] + 1] * phi[i];
      }
      double* uo = d.out_u + ((B * d.S + s) * d.NP + k) * 2;
      uo[0] = ux;
      uo[1] = uy;
      if (k < np1) {
        const double* ps = src.src_p + (int64_t)s * src.src_nv;
        d.out_p[(B * d.S + s) * d.NP1 + k] = ps[dof[0]] * l0 + ps[dof[1]] * l1 + ps[dof[2]] * l2;
      }
    }
    if (d.out_cell) d.out_cell[B * d.NP + k] = best;
  }
}

}  // namespace mdq_mesh

extern "C" int mdq_interpolate_snapshots(const mdq_interp_desc* d, void* stream) {
  if (!d || d->B <= 0 || d->S <= 0 || d->NP <= 0) return mdq_set_error("mdq_interpolate_snapshots: bad arguments");
  int bx = (d->NP + 255) / 256;
  if (d->sparse) {
    if (d->sparse < 0 || d->sparse > 2 || !d->af_facets || !d->naf || !d->cell_dofs || d->NT <= 0 || d->NAF <= 0)
      return mdq_set_error("mdq_interpolate_snapshots: sparse mode needs af_facets, naf, cell_dofs, NT, NAF");
    bx += (3 * d->NAF + 255) / 256;
  }
  if ((d->srcs == nullptr) != (d->src_of_env == nullptr) || (d->srcs && d->n_src <= 0))
    return mdq_set_error("mdq_interpolate_snapshots: srcs and src_of_env go together (n_src > 0)");
  hipLaunchKernelGGL(mdq_mesh::interpolate_kernel, dim3(bx, d->B), dim3(256), 0, (hipStream_t)stream, *d);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mdq_set_error(hipGetErrorString(e));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// State features of B environments (Env2DAirfoil.get_state, Env2DAirfoil.py:282-290), one thread per output value:
//   x[b][n][0:2]        = coordinates()[n_closest[n]]
//   x[b][n][2:2+2S]     = velocities[:, n_closest, :].reshape(N, -1)   (raw row-major reshape of the (S,N,2) block)
//   x[b][n][2+2S:2+3S]  = pressures[:, n_closest][:, :, 0].T
// with the reference's quirk that n_closest (a rank inside the removable list) is used as a VERTEX index; rows
// n >= nsel[b] (fewer than N selectable vertices left) are zero.
namespace mdq_mesh {

__global__ __launch_bounds__(256) void state_features_kernel(int B, int N, int S, int NV, int NP, const double* coords,
                                                             const double* u, const double* p, const int32_t* n_closest,
                                                             const int32_t* nsel, float* x) {
  const int F = 2 + 3 * S;
  const int64_t total = (int64_t)B * N * F;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const int n = (int)((i / F) % N);
    const int b = (int)(i / ((int64_t)F * N));
    const int32_t* nc = n_closest + (int64_t)b * N;
    float val = 0.f;
    if (n < nsel[b]) {
      if (f < 2) {
        val = (float)coords[((int64_t)b * NV + nc[n]) * 2 + f];
      } else if (f < 2 + 2 * S) {
        // element (n, f-2) of the reshaped block = flat index q of the (S, N, 2) array
        const int q = n * 2 * S + (f - 2);
        const int s = q / (2 * N), r = q - s * 2 * N, m = r >> 1, c = r & 1;
        val = (float)u[(((int64_t)b * S + s) * NP + nc[m]) * 2 + c];
      } else {
        const int s = f - 2 - 2 * S;
        val = (float)p[((int64_t)b * S + s) * NV + nc[n]];
      }
    }
    x[i] = val;
  }
}

}  // namespace mdq_mesh

namespace mdq_mesh {
constexpr int RESTORE_MAX = 16;
struct RestoreArgs {
  uint32_t* dst[RESTORE_MAX];
  const uint32_t* src[RESTORE_MAX];
  int64_t words[RESTORE_MAX];
};
// blockIdx.x = position in the index list, blockIdx.y = tensor, blockIdx.z = 16 KB chunk of the row:
// one cached row -> row idx of that tensor, 16 bytes per thread and step where the row allows it
constexpr int RESTORE_CHUNK = 4096;   // words per block
__global__ __launch_bounds__(256) void restore_rows_kernel(RestoreArgs a, const int32_t* idx) {
  const int t = blockIdx.y;
  const int64_t n = a.words[t];
  const int64_t w0 = (int64_t)blockIdx.z * RESTORE_CHUNK;
  if (w0 >= n) return;
  const int64_t w1 = w0 + RESTORE_CHUNK < n ? w0 + RESTORE_CHUNK : n;
  uint32_t* d = a.dst[t] + (int64_t)idx[blockIdx.x] * n;
  const uint32_t* s = a.src[t];
  if ((n & 3) == 0 && ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15) == 0) {
    uint4* d4 = reinterpret_cast<uint4*>(d);
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    for (int64_t i = (w0 >> 2) + threadIdx.x; i < (w1 >> 2); i += 256) d4[i] = s4[i];
  } else {
    for (int64_t i = w0 + threadIdx.x; i < w1; i += 256) d[i] = s[i];
  }
}
}  // namespace mdq_mesh

extern "C" int mdq_restore_rows(int32_t n, void* const* dst, const void* const* src, const int64_t* row_bytes,
                                int32_t n_idx, const int32_t* idx, void* stream) {
  if (n <= 0 || n > mdq_mesh::RESTORE_MAX || !dst || !src || !row_bytes || n_idx < 0 || (n_idx > 0 && !idx))
    return mdq_set_error("mdq_restore_rows: bad arguments (at most 16 tensors)");
  if (n_idx == 0) return 0;
  mdq_mesh::RestoreArgs a;
  for (int t = 0; t < n; ++t) {
    if (!dst[t] || !src[t] || row_bytes[t] <= 0 || (row_bytes[t] & 3) || ((uintptr_t)dst[t] & 3) || ((uintptr_t)src[t] & 3))
      return mdq_set_error("mdq_restore_rows: rows must be non-empty, 4-byte aligned multiples of 4 bytes");
    a.dst[t] = static_cast<uint32_t*>(dst[t]);
    a.src[t] = static_cast<const uint32_t*>(src[t]);
    a.words[t] = row_bytes[t] / 4;
  }
  int64_t wmax = 0;
  for (int t = 0; t < n; ++t) wmax = a.words[t] > wmax ? a.words[t] : wmax;
  const int chunks = (int)((wmax + mdq_mesh::RESTORE_CHUNK - 1) / mdq_mesh::RESTORE_CHUNK);
  hipLaunchKernelGGL(mdq_mesh::restore_rows_kernel, dim3(n_idx, n, chunks), dim3(256), 0, (hipStream_t)stream, a, idx);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("restore_rows_kernel launch failed");
  return 0;
}

namespace mdq_mesh {
// ABI 8: the restores with one cached row per airfoil - row b's source is src[t] + src_of_env[b] * stride[t] words
struct RestoreSrc {
  int64_t stride[RESTORE_MAX];   // words
  const int32_t* src_of_env;
};
__device__ __forceinline__ void restore_one_row(const RestoreArgs& a, const RestoreSrc& r, int t, int64_t row) {
  const int64_t n = a.words[t];
  const int64_t w0 = (int64_t)blockIdx.z * RESTORE_CHUNK;
  if (w0 >= n) return;
  const int64_t w1 = w0 + RESTORE_CHUNK < n ? w0 + RESTORE_CHUNK : n;
  uint32_t* d = a.dst[t] + row * n;
  const uint32_t* s = a.src[t] + (int64_t)__builtin_amdgcn_readfirstlane(r.src_of_env[row]) * r.stride[t];
  if ((n & 3) == 0 && ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15) == 0) {
    uint4* d4 = reinterpret_cast<uint4*>(d);
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    for (int64_t i = (w0 >> 2) + threadIdx.x; i < (w1 >> 2); i += 256) d4[i] = s4[i];
  } else {
    for (int64_t i = w0 + threadIdx.x; i < w1; i += 256) d[i] = s[i];
  }
}
__global__ __launch_bounds__(256) void restore_rows_src_kernel(RestoreArgs a, RestoreSrc r, const int32_t* idx) {
  restore_one_row(a, r, blockIdx.y, idx[blockIdx.x]);
}
__global__ __launch_bounds__(256) void restore_rows_masked_src_kernel(RestoreArgs a, RestoreSrc r, const uint8_t* mask) {
  if (!mask[blockIdx.x]) return;
  restore_one_row(a, r, blockIdx.y, blockIdx.x);
}

// host side of both: the argument checks of mdq_restore_rows + the strides
static int restore_src_args(const char* what, int32_t n, void* const* dst, const void* const* src, const int64_t* src_stride,
                            const int64_t* row_bytes, const int32_t* src_of_env, RestoreArgs& a, RestoreSrc& r, int& chunks) {
  if (n <= 0 || n > RESTORE_MAX || !dst || !src || !src_stride || !row_bytes || !src_of_env)
    return mdq_set_error(what);
  int64_t wmax = 0;
  for (int t = 0; t < n; ++t) {
    if (!dst[t] || !src[t] || row_bytes[t] <= 0 || (row_bytes[t] & 3) || ((uintptr_t)dst[t] & 3) || ((uintptr_t)src[t] & 3) ||
        src_stride[t] < 0 || (src_stride[t] & 3))
      return mdq_set_error(what);
    a.dst[t] = static_cast<uint32_t*>(dst[t]);
    a.src[t] = static_cast<const uint32_t*>(src[t]);
    a.words[t] = row_bytes[t] / 4;
    r.stride[t] = src_stride[t] / 4;
    wmax = a.words[t] > wmax ? a.words[t] : wmax;
  }
  r.src_of_env = src_of_env;
  chunks = (int)((wmax + RESTORE_CHUNK - 1) / RESTORE_CHUNK);
  return 0;
}
}  // namespace mdq_mesh

extern "C" int mdq_restore_rows_src(int32_t n, void* const* dst, const void* const* src, const int64_t* src_stride,
                                    const int64_t* row_bytes, int32_t n_idx, const int32_t* idx, const int32_t* src_of_env,
                                    void* stream) {
  mdq_mesh::RestoreArgs a;
  mdq_mesh::RestoreSrc r;
  int chunks = 0;
  if (n_idx < 0 || (n_idx > 0 && !idx)) return mdq_set_error("mdq_restore_rows_src: bad index list");
  if (mdq_mesh::restore_src_args("mdq_restore_rows_src: bad arguments (at most 16 tensors; rows, strides and pointers multiples "
                                 "of 4 bytes)", n, dst, src, src_stride, row_bytes, src_of_env, a, r, chunks))
    return -1;
  if (n_idx == 0) return 0;
  hipLaunchKernelGGL(mdq_mesh::restore_rows_src_kernel, dim3(n_idx, n, chunks), dim3(256), 0, (hipStream_t)stream, a, r, idx);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("restore_rows_src_kernel launch failed");
  return 0;
}

extern "C" int mdq_restore_rows_masked_src(int32_t n, void* const* dst, const void* const* src, const int64_t* src_stride,
                                           const int64_t* row_bytes, int32_t B, const uint8_t* mask, const int32_t* src_of_env,
                                           void* stream) {
  mdq_mesh::RestoreArgs a;
  mdq_mesh::RestoreSrc r;
  int chunks = 0;
  if (B <= 0 || !mask) return mdq_set_error("mdq_restore_rows_masked_src: bad mask");
  if (mdq_mesh::restore_src_args("mdq_restore_rows_masked_src: bad arguments (at most 16 tensors; rows, strides and pointers "
                                 "multiples of 4 bytes)", n, dst, src, src_stride, row_bytes, src_of_env, a, r, chunks))
    return -1;
  hipLaunchKernelGGL(mdq_mesh::restore_rows_masked_src_kernel, dim3(B, n, chunks), dim3(256), 0, (hipStream_t)stream, a, r, mask);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("restore_rows_masked_src_kernel launch failed");
  return 0;
}

namespace mdq_mesh {
// up to 8 (strided) buffer copies in ONE launch: blockIdx.y = buffer, blockIdx.x walks its rows x 16 KB chunks
struct CopyArgs {
  uint32_t* dst[8];
  const uint32_t* src[8];
  int64_t rows[8], row_words[8], src_stride[8], dst_stride[8];   // strides in words
};
__global__ __launch_bounds__(256) void copy_strided_kernel(CopyArgs a) {
  const int t = blockIdx.y;
  const int64_t rw = a.row_words[t];
  const int64_t chunks = (rw + RESTORE_CHUNK - 1) / RESTORE_CHUNK;
  for (int64_t job = blockIdx.x; job < a.rows[t] * chunks; job += gridDim.x) {
    const int64_t r = job / chunks, c = job - r * chunks;
    const int64_t w0 = c * RESTORE_CHUNK, w1 = w0 + RESTORE_CHUNK < rw ? w0 + RESTORE_CHUNK : rw;
    uint32_t* d = a.dst[t] + r * a.dst_stride[t];
    const uint32_t* s = a.src[t] + r * a.src_stride[t];
    if (((rw | a.dst_stride[t] | a.src_stride[t]) & 3) == 0 && ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15) == 0) {
      uint4* d4 = reinterpret_cast<uint4*>(d);
      const uint4* s4 = reinterpret_cast<const uint4*>(s);
      for (int64_t i = (w0 >> 2) + threadIdx.x; i < (w1 >> 2); i += 256) d4[i] = s4[i];
    } else {
      for (int64_t i = w0 + threadIdx.x; i < w1; i += 256) d[i] = s[i];
    }
  }
}
}  // namespace mdq_mesh

extern "C" int mdq_copy_strided(int32_t n, void* const* dst, const void* const* src, const int64_t* rows,
                                const int64_t* row_bytes, const int64_t* src_stride_bytes, const int64_t* dst_stride_bytes,
                                void* stream) {
  if (n <= 0 || n > 8 || !dst || !src || !rows || !row_bytes || !src_stride_bytes || !dst_stride_bytes)
    return mdq_set_error("mdq_copy_strided: bad arguments (at most 8 buffers)");
  mdq_mesh::CopyArgs a;
  int64_t jobs = 1;
  for (int t = 0; t < 8; ++t) {
    const int q = t < n ? t : 0;
    if (!dst[q] || !src[q] || rows[q] <= 0 || row_bytes[q] <= 0 || ((row_bytes[q] | src_stride_bytes[q] | dst_stride_bytes[q]) & 3) ||
        (((uintptr_t)dst[q] | (uintptr_t)src[q]) & 3))
      return mdq_set_error("mdq_copy_strided: rows and strides must be non-empty, 4-byte aligned multiples of 4 bytes");
    a.dst[t] = static_cast<uint32_t*>(dst[q]);
    a.src[t] = static_cast<const uint32_t*>(src[q]);
    a.rows[t] = rows[q];
    a.row_words[t] = row_bytes[q] / 4;
    a.src_stride[t] = src_stride_bytes[q] / 4;
    a.dst_stride[t] = dst_stride_bytes[q] / 4;
    const int64_t j = a.rows[t] * ((a.row_words[t] + mdq_mesh::RESTORE_CHUNK - 1) / mdq_mesh::RESTORE_CHUNK);
    jobs = j > jobs ? j : jobs;
  }
  const int gx = (int)(jobs < 1024 ? jobs : 1024);
  hipLaunchKernelGGL(mdq_mesh::copy_strided_kernel, dim3(gx, n), dim3(256), 0, (hipStream_t)stream, a);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("copy_strided_kernel launch failed");
  return 0;
}

namespace mdq_mesh {
// blockIdx.x = environment: its first edge_ptr[b+1] - edge_ptr[b] padded entries -> the packed lists
__global__ __launch_bounds__(256) void compact_edges_kernel(int EMAX, const int32_t* __restrict__ src_pad,
                                                             const int32_t* __restrict__ dst_pad,
                                                             const int32_t* __restrict__ edge_ptr, int32_t* __restrict__ esrc,
                                                             int32_t* __restrict__ edst) {
  const int b = blockIdx.x, e0 = edge_ptr[b], n = edge_ptr[b + 1] - e0;
  const int32_t* s = src_pad + (int64_t)b * EMAX;
  const int32_t* d = dst_pad + (int64_t)b * EMAX;
  for (int i = threadIdx.x; i < n; i += 256) {
    esrc[e0 + i] = s[i];
    edst[e0 + i] = d[i];
  }
}
}  // namespace mdq_mesh

extern "C" int mdq_compact_edges(int32_t B, int32_t EMAX, const int32_t* src_pad, const int32_t* dst_pad,
                                 const int32_t* edge_ptr, int32_t* esrc, int32_t* edst, void* stream) {
  if (B <= 0 || EMAX <= 0 || !src_pad || !dst_pad || !edge_ptr || !esrc || !edst)
    return mdq_set_error("mdq_compact_edges: bad arguments");
  hipLaunchKernelGGL(mdq_mesh::compact_edges_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, EMAX, src_pad, dst_pad,
                     edge_ptr, esrc, edst);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("compact_edges_kernel launch failed");
  return 0;
}

extern "C" int mdq_state_features(int32_t B, int32_t N, int32_t S, int32_t NV, int32_t NP, const double* coords,
                                  const double* u, const double* p, const int32_t* n_closest, const int32_t* nsel,
                                  float* x, void* stream) {
  if (B <= 0 || N <= 0 || S <= 0 || !coords || !u || !p || !n_closest || !nsel || !x)
    return mdq_set_error("mdq_state_features: bad arguments");
  const int64_t total = (int64_t)B * N * (2 + 3 * S);
  const int blocks = (int)((total + 255) / 256);
  hipLaunchKernelGGL(mdq_mesh::state_features_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, B, N, S, NV, NP,
                     coords, u, p, n_closest, nsel, x);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("state_features_kernel launch failed");
  return 0;
}

// ================================================================== control logic of the batched env step on the device
//
// `VecEnv2DAirfoil.step` (Env2DAirfoil.step, Env2DAirfoil.py:318-377; calculate_reward :380-428) decides four things
// per environment: which vertex an action removes, how often the smoothing runs, reward + terminal flag, and which
// environments restart.  With these kernels the decisions stay on the device, so that a rollout is one uninterrupted
// stream of launches: no read-back between the Q-network forward and the next vertex removal.
namespace mdq_mesh {

// one wave per environment: greedy action = first maximum of q[b][0..NA) (torch.argmax), epsilon-greedy choice, then
// Env2DAirfoil.step's action decoding: N = "do nothing" (shift the N-closest window), an action without a vertex
// behind it = code 2 ("RAN OUT OF VERTICES"), otherwise the vertex id coord_map[b][action]
__global__ __launch_bounds__(64) void env_act_kernel(int N, const float* q, const uint8_t* explore, const int32_t* rand_action,
                                                      const int32_t* nsel, const int32_t* coord_map, int32_t* offset,
                                                      int32_t* action, int32_t* rem, int32_t* code) {
  const int b = blockIdx.x, lane = threadIdx.x, NA = N + 1;
  int a;
  if (q) {
    float best = -__builtin_inff();
    int bi = 0x7FFFFFFF;
    for (int i = lane; i < NA; i += 64) {
      const float v = q[(int64_t)b * NA + i];
      if (v > best || (v == best && i < bi) || (bi == 0x7FFFFFFF && !(v < best))) {   // (NaN rows: first index)
        best = v;
        bi = i;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best, off);
      const int oi = __shfl_xor(bi, off);
      if (ov > best || (ov == best && oi < bi)) {
        best = ov;
        bi = oi;
      }
    }
    a = (explore && explore[b]) ? rand_action[b] : bi;
  } else {
    a = action[b];
  }
  if (lane == 0) {
    const bool shift = a == N;
    const bool pick = a >= 0 && a < nsel[b] && !shift;
    if (shift) offset[b] += 1;
    action[b] = a;
    rem[b] = pick ? coord_map[(int64_t)b * N + min(max(a, 0), N - 1)] : -1;
    code[b] = (!shift && !pick) ? 2 : 0;
  }
}

__global__ void env_smooth_iters_kernel(int B, const int32_t* rem, const int32_t* rstat, int32_t iterations, int32_t* its) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) its[b] = (rem[b] >= 0 && rstat[b] == 0) ? iterations : 0;
}

// reward / terminal flag (Env2DAirfoil.calculate_reward + the bookkeeping of step()): one thread per environment.
// Codes as in Env2DAirfoil.py:342-364: 0 = removed (reward from calculate_reward), 1 = "already removed" (reward -1, NOT
// terminal), 2 = broken / out of vertices (reward -1, terminal).  The reference's _remove_vertex / _check_mesh only ever
// return 0 or 2 (:458,:491,:573,:587,:598,:602) and nothing here produces 1 either; the branch is kept for parity.
// new_lifts / gt_lift (both or neither; not in the reference, whose calculate_reward fills new_lifts and ignores them): the
// lift part of the reward and of the accuracy stop, header: mdq_env_result_forces.  NULL: the drag-only step, bit for bit.
__global__ void env_result_kernel(int B, int N, int S, const double* new_drags, const double* gt_drag, const int32_t* nv,
                                  int32_t nv0, const int32_t* rstat, const int32_t* topo_status, const int32_t* nsel,
                                  int32_t* code, int32_t* steps, double threshold, double time_reward, double goal_vertices,
                                  int32_t timesteps, double negative_reward, int32_t auto_reset, double* reward,
                                  uint8_t* done, int32_t* err_flag, int32_t* nv_out, const double* new_lifts,
                                  const double* gt_lift, double lift_weight, double lift_threshold, double lift_floor,
                                  int32_t* reason, const double* quality, const double* quality_ref, double quality_weight,
                                  double min_quality, double max_cot) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int c = code[b];
  if (rstat[b] != 0 || nsel[b] < N) c = 2;
  if (topo_status && topo_status[b] != 0) {
    c = 2;
    atomicOr(err_flag, 1);
  }
  const double drag_factor = -2.0 * log(0.5) / threshold;
  double ss = 0.0;
  bool acc = false;
  for (int s = 0; s < S; ++s) {
    const double g = gt_drag[s], d = new_drags[(int64_t)b * S + s];
    const double e = fabs(g - d) / fabs(g);
    ss += e * e;
    acc = acc || fabs(fabs(g - d) / g) > threshold;
  }
  const double drag_reward = 2.0 * exp(-drag_factor * sqrt(ss)) - 1.0;
  const double tr = (double)(nv0 - nv[b]) * time_reward;
  const bool vert = (double)nv[b] < goal_vertices * (double)nv0;
  const bool ok = c == 0;
  double r_ok = drag_reward + tr, num = drag_reward, den = 1.0;
  bool accl = false, accq = false;
  if (new_lifts) {
    const double lift_factor = -2.0 * log(0.5) / lift_threshold;
    double sl = 0.0;
    for (int s = 0; s < S; ++s) {
      const double g = gt_lift[s], l = new_lifts[(int64_t)b * S + s];
      const double el = fabs(g - l) / fmax(fabs(g), lift_floor);
      sl += el * el;
      accl = accl || el > lift_threshold;
    }
    const double lift_reward = 2.0 * exp(-lift_factor * sqrt(sl)) - 1.0;
    num = drag_reward + lift_weight * lift_reward;
    den = 1.0 + lift_weight;
    r_ok = num / den + tr;
  }
  if (quality) {        // (header: mdq_env_result_quality)
    const double q_min = quality[2 * (int64_t)b], cot_max = quality[2 * (int64_t)b + 1];
    const double quality_reward = 2.0 * fmin(q_min / quality_ref[0], 1.0) - 1.0;
    accq = q_min < min_quality || cot_max > max_cot;
    num = num + quality_weight * quality_reward;
    den = den + quality_weight;
    r_ok = num / den + tr;
  }
  double r = ok ? r_ok : negative_reward;
  bool dn = ok ? (acc || accl || accq || vert) : (c != 1);
  const int st = steps[b] + 1;
  dn = dn || st >= timesteps;
  reward[b] = r;
  if (nv_out) nv_out[b] = nv[b];      // (the vertex count of the step, before an in-place reset rewrites nv)
  done[b] = dn ? 1 : 0;
  if (reason)
    reason[b] = (ok ? (acc ? 1 : 0) | (accl ? 2 : 0) | (vert ? 4 : 0) | (accq ? 32 : 0) : (c != 1 ? 8 : 0)) |
                (st >= timesteps ? 16 : 0);
  code[b] = c;
  steps[b] = (dn && auto_reset) ? 0 : st;
}

__global__ __launch_bounds__(256) void restore_rows_masked_kernel(RestoreArgs a, const uint8_t* mask) {
  if (!mask[blockIdx.x]) return;
  const int t = blockIdx.y;
  const int64_t n = a.words[t];
  const int64_t w0 = (int64_t)blockIdx.z * RESTORE_CHUNK;
  if (w0 >= n) return;
  const int64_t w1 = w0 + RESTORE_CHUNK < n ? w0 + RESTORE_CHUNK : n;
  uint32_t* d = a.dst[t] + (int64_t)blockIdx.x * n;
  const uint32_t* s = a.src[t];
  if ((n & 3) == 0 && ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s)) & 15) == 0) {
    uint4* d4 = reinterpret_cast<uint4*>(d);
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    for (int64_t i = (w0 >> 2) + threadIdx.x; i < (w1 >> 2); i += 256) d4[i] = s4[i];
  } else {
    for (int64_t i = w0 + threadIdx.x; i < w1; i += 256) d[i] = s[i];
  }
}

// edge_ptr = exclusive prefix sums of nedges (one block; B <= 1024 per launch is plenty: environments per GPU)
__global__ __launch_bounds__(1024) void edge_ptr_kernel(int B, const int32_t* nedges, int32_t* edge_ptr) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  int run = 0;
  for (int base = 0; base < B; base += 1024) {
    const int i = base + tid;
    part[tid] = i < B ? nedges[i] : 0;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int add = tid >= off ? part[tid - off] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    if (i < B) edge_ptr[i + 1] = run + part[tid];
    run += part[1023];
    __syncthreads();
  }
  if (tid == 0) edge_ptr[0] = 0;
}

}  // namespace mdq_mesh

extern "C" int mdq_env_act(int32_t B, int32_t N, const float* q, const uint8_t* explore, const int32_t* rand_action,
                           const int32_t* nsel, const int32_t* coord_map, int32_t* offset, int32_t* action, int32_t* rem,
                           int32_t* code, void* stream) {
  if (B <= 0 || N <= 0 || !nsel || !coord_map || !offset || !action || !rem || !code || (explore && !rand_action))
    return mdq_set_error("mdq_env_act: bad arguments");
  hipLaunchKernelGGL(mdq_mesh::env_act_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, N, q, explore, rand_action, nsel,
                     coord_map, offset, action, rem, code);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("env_act_kernel launch failed");
  return 0;
}

extern "C" int mdq_env_smooth_iters(int32_t B, const int32_t* rem, const int32_t* rstat, int32_t iterations, int32_t* its,
                                    void* stream) {
  if (B <= 0 || !rem || !rstat || !its) return mdq_set_error("mdq_env_smooth_iters: bad arguments");
  hipLaunchKernelGGL(mdq_mesh::env_smooth_iters_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, rem, rstat,
                     iterations, its);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("env_smooth_iters_kernel launch failed");
  return 0;
}

// the lift arguments of mdq_env_result_forces / mdq_env_finish_desc: NULL when they are acceptable (both arrays absent, or
// both present with w >= 0 finite, T > 0 (+inf allowed), F >= 0 finite), else what is wrong with them
static const char* lift_args_error(const double* new_lifts, const double* gt_lift, double w, double T, double F) {
  if ((new_lifts == nullptr) != (gt_lift == nullptr)) return "new_lifts and gt_lift go together (both or neither)";
  if (!new_lifts) return nullptr;
  if (!(w >= 0.0) || std::isinf(w)) return "lift_weight must be finite and >= 0";
  if (!(T > 0.0)) return "lift_threshold must be > 0 (+inf: no lift stop)";
  if (!(F >= 0.0) || std::isinf(F)) return "lift_floor must be finite and >= 0";
  return nullptr;
}

// the quality arguments of mdq_env_result_quality / mdq_env_finish_desc: NULL when they are acceptable (both arrays absent,
// or both present with wq >= 0 finite, Qm in [0, 1), max_cot > 0 (+inf allowed)), else what is wrong with them
static const char* quality_args_error(const double* quality, const double* quality_ref, double wq, double Qm, double max_cot) {
  if ((quality == nullptr) != (quality_ref == nullptr)) return "quality and quality_ref go together (both or neither)";
  if (!quality) return nullptr;
  if (!(wq >= 0.0) || std::isinf(wq)) return "quality_weight must be finite and >= 0";
  if (!(Qm >= 0.0 && Qm < 1.0)) return "min_quality must lie in [0, 1) (0: no stop)";
  if (!(max_cot > 0.0)) return "max_cot must be > 0 (+inf: no angle stop)";
  return nullptr;
}

extern "C" int mdq_env_result_quality(int32_t B, int32_t N, int32_t S, const double* new_drags, const double* gt_drag,
                                      const int32_t* nv, int32_t nv0, const int32_t* rstat, const int32_t* topo_status,
                                      const int32_t* nsel, int32_t* code, int32_t* steps, double threshold, double time_reward,
                                      double goal_vertices, int32_t timesteps, double negative_reward, int32_t auto_reset,
                                      double* reward, uint8_t* done, int32_t* err_flag, int32_t* nv_out, const double* new_lifts,
                                      const double* gt_lift, double lift_weight, double lift_threshold, double lift_floor,
                                      int32_t* reason, const double* quality, const double* quality_ref, double quality_weight,
                                      double min_quality, double max_cot, void* stream) {
  if (B <= 0 || S <= 0 || !new_drags || !gt_drag || !nv || !rstat || !nsel || !code || !steps || !reward || !done || !err_flag)
    return mdq_set_error("mdq_env_result: bad arguments");
  if (const char* why = lift_args_error(new_lifts, gt_lift, lift_weight, lift_threshold, lift_floor))
    return mdq_set_error((std::string("mdq_env_result_forces: ") + why).c_str());
  if (const char* why = quality_args_error(quality, quality_ref, quality_weight, min_quality, max_cot))
    return mdq_set_error((std::string("mdq_env_result_quality: ") + why).c_str());
  hipLaunchKernelGGL(mdq_mesh::env_result_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, B, N, S, new_drags,
                     gt_drag, nv, nv0, rstat, topo_status, nsel, code, steps, threshold, time_reward, goal_vertices, timesteps,
                     negative_reward, auto_reset, reward, done, err_flag, nv_out, new_lifts, gt_lift, lift_weight, lift_threshold,
                     lift_floor, reason, quality, quality_ref, quality_weight, min_quality, max_cot);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("env_result_kernel launch failed");
  return 0;
}

extern "C" int mdq_env_result_forces(int32_t B, int32_t N, int32_t S, const double* new_drags, const double* gt_drag,
                                     const int32_t* nv, int32_t nv0, const int32_t* rstat, const int32_t* topo_status,
                                     const int32_t* nsel, int32_t* code, int32_t* steps, double threshold, double time_reward,
                                     double goal_vertices, int32_t timesteps, double negative_reward, int32_t auto_reset,
                                     double* reward, uint8_t* done, int32_t* err_flag, int32_t* nv_out, const double* new_lifts,
                                     const double* gt_lift, double lift_weight, double lift_threshold, double lift_floor,
                                     int32_t* reason, void* stream) {
  return mdq_env_result_quality(B, N, S, new_drags, gt_drag, nv, nv0, rstat, topo_status, nsel, code, steps, threshold, time_reward,
                                goal_vertices, timesteps, negative_reward, auto_reset, reward, done, err_flag, nv_out, new_lifts,
                                gt_lift, lift_weight, lift_threshold, lift_floor, reason, nullptr, nullptr, 0.0, 0.0, 0.0, stream);
}

extern "C" int mdq_env_result(int32_t B, int32_t N, int32_t S, const double* new_drags, const double* gt_drag, const int32_t* nv,
                              int32_t nv0, const int32_t* rstat, const int32_t* topo_status, const int32_t* nsel,
                              int32_t* code, int32_t* steps, double threshold, double time_reward, double goal_vertices,
                              int32_t timesteps, double negative_reward, int32_t auto_reset, double* reward, uint8_t* done,
                              int32_t* err_flag, int32_t* nv_out, void* stream) {
  return mdq_env_result_forces(B, N, S, new_drags, gt_drag, nv, nv0, rstat, topo_status, nsel, code, steps, threshold, time_reward,
                               goal_vertices, timesteps, negative_reward, auto_reset, reward, done, err_flag, nv_out, nullptr,
                               nullptr, 0.0, 0.0, 0.0, nullptr, stream);
}

extern "C" int mdq_restore_rows_masked(int32_t n, void* const* dst, const void* const* src, const int64_t* row_bytes,
                                       int32_t B, const uint8_t* mask, void* stream) {
  if (n <= 0 || n > mdq_mesh::RESTORE_MAX || !dst || !src || !row_bytes || B <= 0 || !mask)
    return mdq_set_error("mdq_restore_rows_masked: bad arguments (at most 16 tensors)");
  mdq_mesh::RestoreArgs a;
  for (int t = 0; t < n; ++t) {
    if (!dst[t] || !src[t] || row_bytes[t] <= 0 || (row_bytes[t] & 3) || ((uintptr_t)dst[t] & 3) || ((uintptr_t)src[t] & 3))
      return mdq_set_error("mdq_restore_rows_masked: rows must be non-empty, 4-byte aligned multiples of 4 bytes");
    a.dst[t] = static_cast<uint32_t*>(dst[t]);
    a.src[t] = static_cast<const uint32_t*>(src[t]);
    a.words[t] = row_bytes[t] / 4;
  }
  int64_t wmax = 0;
  for (int t = 0; t < n; ++t) wmax = a.words[t] > wmax ? a.words[t] : wmax;
  const int chunks = (int)((wmax + mdq_mesh::RESTORE_CHUNK - 1) / mdq_mesh::RESTORE_CHUNK);
  hipLaunchKernelGGL(mdq_mesh::restore_rows_masked_kernel, dim3(B, n, chunks), dim3(256), 0, (hipStream_t)stream, a, mask);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("restore_rows_masked_kernel launch failed");
  return 0;
}

namespace mdq_mesh {
// The end of a device-resident env step in one launch: blockIdx.x = environment, blockIdx.y = one of gridDim.y workgroups
// that share its copy work (result logic: computed by every workgroup from the *_in arrays, written by y = 0).
// The terminal decision reads nv[b] and nsel[b], which are ALSO row arrays this launch resets in place: a workgroup (b, y)
// that started after another one had restored them would decide "not terminal" and skip its share of the rows - a
// half-reset environment (round 4's kernel: harmless only while all B Y workgroups were co-resident).  So the rows whose
// destination is d.nv / d.nsel are kept out of the strided restore: every workgroup of a resetting environment arrives
// at a counter when it has finished READING (decision + hand-over copies), and the LAST one to arrive restores them and
// puts the counter back to zero - no workgroup waits for another.
__global__ __launch_bounds__(256) void env_finish_kernel(mdq_env_finish_desc d) {
  const int b = blockIdx.x, y = blockIdx.y, Y = gridDim.y, tid = threadIdx.x;
  // airfoil of this environment (a batch over several airfoils; workgroup-uniform): its ground truth, initial vertex count,
  // cached initial rows and features
  const int a = d.src_of_env ? __builtin_amdgcn_readfirstlane(d.src_of_env[b]) : 0;
  const double* gt_drag = d.gt_drag + (int64_t)a * d.S;
  const int nv0 = d.src_of_env ? d.nv0_of[a] : d.nv0;
  __shared__ int s_reset;
  if (tid == 0) {
#pragma clang fp contract(off)
    // ---- 1. mdq_env_result for environment b (same operations in the same order)
    int c = d.code_in[b];
    if (d.rstat[b] != 0 || d.nsel[b] < d.N) c = 2;
    if (d.topo_status && d.topo_status[b] != 0) {
      c = 2;
      if (y == 0) atomicOr(d.err_flag, 1);
    }
    const double drag_factor = -2.0 * log(0.5) / d.threshold;
    double ss = 0.0;
    bool acc = false;
    for (int s = 0; s < d.S; ++s) {
      const double g = gt_drag[s], dr = d.new_drags[(int64_t)b * d.S + s];
      const double e = fabs(g - dr) / fabs(g);
      ss += e * e;
      acc = acc || fabs(fabs(g - dr) / g) > d.threshold;
    }
    const double drag_reward = 2.0 * exp(-drag_factor * sqrt(ss)) - 1.0;
    const int nvb = d.nv[b];
    const double tr = (double)(nv0 - nvb) * d.time_reward;
    const bool vert = (double)nvb < d.goal_vertices * (double)nv0;
    const bool ok = c == 0;
    double r_ok = drag_reward + tr, num = drag_reward, den = 1.0;
    bool accl = false, accq = false;
    if (d.new_lifts) {       // (workgroup-uniform: a kernel argument)
      const double* gt_lift = d.gt_lift + (int64_t)a * d.S;
      const double lift_factor = -2.0 * log(0.5) / d.lift_threshold;
      double sl = 0.0;
      for (int s = 0; s < d.S; ++s) {
        const double g = gt_lift[s], l = d.new_lifts[(int64_t)b * d.S + s];
        const double el = fabs(g - l) / fmax(fabs(g), d.lift_floor);
        sl += el * el;
        accl = accl || el > d.lift_threshold;
      }
      const double lift_reward = 2.0 * exp(-lift_factor * sqrt(sl)) - 1.0;
      num = drag_reward + d.lift_weight * lift_reward;
      den = 1.0 + d.lift_weight;
      r_ok = num / den + tr;
    }
    if (d.quality) {         // (workgroup-uniform: a kernel argument; header: mdq_env_result_quality)
      const double q_min = d.quality[2 * (int64_t)b], cot_max = d.quality[2 * (int64_t)b + 1];
      const double quality_reward = 2.0 * fmin(q_min / d.quality_ref[a], 1.0) - 1.0;
      accq = q_min < d.min_quality || cot_max > d.max_cot;
      num = num + d.quality_weight * quality_reward;
      den = den + d.quality_weight;
      r_ok = num / den + tr;
    }
    const double r = ok ? r_ok : d.negative_reward;
    bool dn = ok ? (acc || accl || accq || vert) : (c != 1);
    const int st = d.steps_in[b] + 1;
    dn = dn || st >= d.timesteps;
    if (y == 0) {
      d.reward[b] = r;
      if (d.nv_out) d.nv_out[b] = nvb;
      d.done[b] = dn ? 1 : 0;
      if (d.reason)
        d.reason[b] = (ok ? (acc ? 1 : 0) | (accl ? 2 : 0) | (vert ? 4 : 0) | (accq ? 32 : 0) : (c != 1 ? 8 : 0)) |
                      (st >= d.timesteps ? 16 : 0);
      d.code_out[b] = c;
      d.steps_out[b] = (dn && d.auto_reset) ? 0 : st;
    }
    s_reset = (dn && d.auto_reset) ? 1 : 0;
  }
  __syncthreads();
  const bool reset = s_reset != 0;
  // ---- 2. hand-over of the pre-reset rows, then the in-place reset: word i of a row is read once, copied out if it lies
  // in the hand-over window, then overwritten (same thread: no ordering problem between the two)
  const int lin = y * 256 + tid, nlin = Y * 256;
  for (int t = 0; t < d.n_rows; ++t) {
    uint32_t* ho = static_cast<uint32_t*>(d.handover_dst[t]);
    const uint32_t* src = static_cast<const uint32_t*>(d.src[t]);
    if (src && d.src_of_env) src += (a * d.src_stride[t]) >> 2;
    const bool late = d.dst[t] == static_cast<const void*>(d.nv) || d.dst[t] == static_cast<const void*>(d.nsel);
    const bool restore = reset && src != nullptr && !late;
    if (!ho && !restore) continue;
    const int64_t words = d.row_bytes[t] >> 2, h0 = d.handover_off[t] >> 2, hw = d.handover_bytes[t] >> 2;
    uint32_t* row = static_cast<uint32_t*>(d.dst[t]) + (int64_t)b * words;
    uint32_t* hob = ho ? ho + (int64_t)b * hw : nullptr;
    const int64_t lo = restore ? 0 : h0, hi = restore ? words : h0 + hw;
    const bool vec = ((words | h0 | hw) & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(row) | reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(hob)) & 15) == 0;
    if (vec) {
      uint4* row4 = reinterpret_cast<uint4*>(row);
      const uint4* src4 = reinterpret_cast<const uint4*>(src);
      uint4* ho4 = reinterpret_cast<uint4*>(hob);
      const int64_t h04 = h0 >> 2, h14 = (h0 + hw) >> 2;
      for (int64_t i = (lo >> 2) + lin; i < (hi >> 2); i += nlin) {
        if (ho && i >= h04 && i < h14) ho4[i - h04] = row4[i];
        if (restore) row4[i] = src4[i];
      }
    } else {
      for (int64_t i = lo + lin; i < hi; i += nlin) {
        if (ho && i >= h0 && i < h0 + hw) hob[i - h0] = row[i];
        if (restore) row[i] = src[i];
      }
    }
  }
  // ---- 2b. the decision's own inputs (nv, nsel): restored by the last workgroup of the environment to get here
  if (reset) {
    __syncthreads();                                   // this workgroup's hand-over reads are done
    if (tid == 0) {
      bool last = true;
      if (Y > 1) {
        __threadfence();
        last = atomicAdd(d.arrive + b, 1) == Y - 1;
      }
      if (last) {
        for (int t = 0; t < d.n_rows; ++t) {
          const uint32_t* src = static_cast<const uint32_t*>(d.src[t]);
          if (!src || (d.dst[t] != static_cast<const void*>(d.nv) && d.dst[t] != static_cast<const void*>(d.nsel))) continue;
          if (d.src_of_env) src += (a * d.src_stride[t]) >> 2;
          const int64_t words = d.row_bytes[t] >> 2;
          uint32_t* row = static_cast<uint32_t*>(d.dst[t]) + (int64_t)b * words;
          for (int64_t i = 0; i < words; ++i) row[i] = src[i];
        }
        if (Y > 1) d.arrive[b] = 0;                     // the next launch finds the counter at zero again
      }
    }
  }
  // ---- 3. node features of the next state (state_features_kernel's formulas); a reset environment: the cached ones
  const int N = d.N, S = d.S, F = 2 + 3 * S;
  float* xb = d.x + (int64_t)b * N * F;
  if (reset && d.x_init) {
    const float* xi = d.x_init + (int64_t)a * N * F;
    for (int i = lin; i < N * F; i += nlin) xb[i] = xi[i];
    return;
  }
  if (reset) {               // (no cached features: read the rows restored above - needs all of them: one workgroup only)
    __threadfence_block();
    __syncthreads();
  }
  const int32_t* nc = d.n_closest + (int64_t)b * N;
  const int nselb = d.nsel[b];
  for (int i = lin; i < N * F; i += nlin) {
    const int n = i / F, f = i - n * F;
    float val = 0.f;
    if (n < nselb) {
      if (f < 2) {
        val = (float)d.coords[((int64_t)b * d.NV + nc[n]) * 2 + f];
      } else if (f < 2 + 2 * S) {
        const int q = n * 2 * S + (f - 2);
        const int s = q / (2 * N), r = q - s * 2 * N, m = r >> 1, c = r & 1;
        val = (float)d.u[(((int64_t)b * S + s) * d.NP + nc[m]) * 2 + c];
      } else {
        const int s = f - 2 - 2 * S;
        val = (float)d.p[((int64_t)b * S + s) * d.NV + nc[n]];
      }
    }
    xb[i] = val;
  }
}
}  // namespace mdq_mesh

extern "C" int mdq_env_finish(const mdq_env_finish_desc* d, void* stream) {
  if (!d || d->B <= 0 || d->N <= 0 || d->S <= 0 || d->n_rows < 0 || d->n_rows > MDQ_FINISH_MAX_ROWS || !d->new_drags ||
      !d->gt_drag || !d->nv || !d->rstat || !d->nsel || !d->code_in || !d->code_out || !d->steps_in || !d->steps_out ||
      d->steps_in == d->steps_out || !d->reward || !d->done || !d->err_flag || !d->coords || !d->u || !d->p || !d->n_closest || !d->x)
    return mdq_set_error("mdq_env_finish: bad arguments");
  int64_t bytes = 0;
  for (int t = 0; t < d->n_rows; ++t) {
    if (!d->dst[t] || d->row_bytes[t] <= 0 || ((d->row_bytes[t] | d->handover_off[t] | d->handover_bytes[t]) & 3) ||
        (((uintptr_t)d->dst[t] | (uintptr_t)d->src[t] | (uintptr_t)d->handover_dst[t]) & 3) ||
        (d->handover_dst[t] && (d->handover_off[t] < 0 || d->handover_bytes[t] <= 0 ||
                                d->handover_off[t] + d->handover_bytes[t] > d->row_bytes[t])))
      return mdq_set_error("mdq_env_finish: rows must be non-empty 4-byte aligned multiples of 4 bytes with a hand-over window inside them");
    bytes += d->handover_dst[t] ? d->handover_bytes[t] : 0;
    if (d->src_of_env && (d->src_stride[t] < 0 || (d->src_stride[t] & 3)))
      return mdq_set_error("mdq_env_finish: src_stride must be a non-negative multiple of 4 bytes");
  }
  if (d->src_of_env && !d->nv0_of) return mdq_set_error("mdq_env_finish: src_of_env needs nv0_of");
  if (const char* why = lift_args_error(d->new_lifts, d->gt_lift, d->lift_weight, d->lift_threshold, d->lift_floor))
    return mdq_set_error((std::string("mdq_env_finish: ") + why).c_str());
  if (const char* why = quality_args_error(d->quality, d->quality_ref, d->quality_weight, d->min_quality, d->max_cot))
    return mdq_set_error((std::string("mdq_env_finish: ") + why).c_str());
  // workgroups per environment: enough lanes for the hand-over copies AND the in-place reset of a terminated environment
  // (16 bytes per lane and pass, ~4 passes; the workgroups of the other environments find nothing to restore and leave);
  // without cached initial features the reset path needs the whole environment in one workgroup
  int64_t rbytes = 0;
  for (int t = 0; t < d->n_rows; ++t) rbytes += (d->auto_reset && d->src[t]) ? d->row_bytes[t] : 0;
  if (rbytes > bytes) bytes = rbytes;
  int Y = (int)((bytes / 16 + 1023) / 1024);
  Y = Y < 1 ? 1 : (Y > 16 ? 16 : Y);
  if (d->auto_reset && !d->x_init) Y = 1;
  if (d->auto_reset && Y > 1 && !d->arrive) {
    // (a caller without the counter array keeps one workgroup per environment: slower for large rows, never wrong)
    Y = 1;
  }
  hipLaunchKernelGGL(mdq_mesh::env_finish_kernel, dim3(d->B, Y), dim3(256), 0, (hipStream_t)stream, *d);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("env_finish_kernel launch failed");
  return 0;
}

namespace mdq_mesh {
// ---- shape quality of the cells (header: mdq_mesh_quality; not in the reference)
// (value, index) pairs: `(v2, i2)` replaces `(v, i)` when its value is better (LESS: smaller, else larger) or equal with the
// lower index - an order-independent choice, so the lanes and waves may be combined in any order.  No NaN enters: a cell
// whose numbers are not finite has been turned into the worst cell before.
template <bool LESS>
__device__ __forceinline__ void qpair_take(double& v, int& i, double v2, int i2) {
  const bool better = LESS ? v2 < v : v2 > v;
  if (better || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// One 256-thread workgroup per environment, thread t walks the cells t, t + 256, ...; the mesh size appears in the trip
// count only (no LDS table, no atomics), so the one instance serves every mesh class.
__global__ __launch_bounds__(256) void mesh_quality_kernel(int NV, int NT, const double* __restrict__ coords,
                                                           const int32_t* __restrict__ cells, const int32_t* __restrict__ nv,
                                                           const int32_t* __restrict__ nt, double q_floor,
                                                           double* __restrict__ qual, int32_t* __restrict__ qinfo) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nvb = max(min(__builtin_amdgcn_readfirstlane(nv[b]), NV), 0);
  const int ntb = min(__builtin_amdgcn_readfirstlane(nt[b]), NT);
  const double INF = __builtin_inf();
  if (ntb <= 0) {        // (workgroup-uniform)
    if (tid == 0) {
      *reinterpret_cast<double2*>(qual + 2 * (int64_t)b) = make_double2(0.0, INF);
      *reinterpret_cast<int4*>(qinfo + 4 * (int64_t)b) = make_int4(-1, -1, 0, 0);
    }
    return;
  }
  const double2* P = reinterpret_cast<const double2*>(coords) + (int64_t)b * NV;      // (one 16-byte load per vertex)
  const int32_t* C = cells + (int64_t)b * NT * 3;
  const double K = 3.4641016151377544;       // 2 sqrt(3)
  double bq = INF, bc = -INF;
  int iq = INT_MAX, ic = INT_MAX, cnt = 0;
  for (int t = tid; t < ntb; t += 256) {
    const int i0 = C[3 * t], i1 = C[3 * t + 1], i2 = C[3 * t + 2];
    double q = 0.0, cot = INF;
    if ((unsigned)i0 < (unsigned)nvb && (unsigned)i1 < (unsigned)nvb && (unsigned)i2 < (unsigned)nvb) {
      const double2 p0 = P[i0], p1 = P[i1], p2 = P[i2];
      const double ax = p1.x - p0.x, ay = p1.y - p0.y, bx = p2.x - p0.x, by = p2.y - p0.y, cx = p2.x - p1.x, cy = p2.y - p1.y;
      const double A2 = fabs((ax * by) - (ay * bx));
      const double s = ((ax * ax + ay * ay) + (bx * bx + by * by)) + (cx * cx + cy * cy);
      const double qc = s > 0.0 ? (K * A2) / s : 0.0;
      const double d0 = ax * bx + ay * by, d1 = -(ax * cx + ay * cy), d2 = bx * cx + by * cy;
      const double cc = A2 > 0.0 ? fmax(d0, fmax(d1, d2)) / A2 : INF;
      if (fabs(qc) < INF && fabs(cc) < INF) {       // (both finite; else the worst cell)
        q = qc;
        cot = cc;
      }
    }
    if (q < bq) {         // (t ascends: the first cell to attain a value keeps it)
      bq = q;
      iq = t;
    }
    if (cot > bc) {
      bc = cot;
      ic = t;
    }
    cnt += q < q_floor ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    qpair_take<true>(bq, iq, __shfl_xor(bq, o, 64), __shfl_xor(iq, o, 64));
    qpair_take<false>(bc, ic, __shfl_xor(bc, o, 64), __shfl_xor(ic, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  __shared__ double s_q[4], s_c[4];
  __shared__ int s_iq[4], s_ic[4], s_cnt[4];
  const int w = tid >> 6;
  if ((tid & 63) == 0) {
    s_q[w] = bq, s_iq[w] = iq;
    s_c[w] = bc, s_ic[w] = ic;
    s_cnt[w] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k) {
      qpair_take<true>(bq, iq, s_q[k], s_iq[k]);
      qpair_take<false>(bc, ic, s_c[k], s_ic[k]);
      cnt += s_cnt[k];
    }
    *reinterpret_cast<double2*>(qual + 2 * (int64_t)b) = make_double2(bq, bc);
    *reinterpret_cast<int4*>(qinfo + 4 * (int64_t)b) = make_int4(iq, ic, cnt, 0);
  }
}
}  // namespace mdq_mesh

extern "C" int mdq_mesh_quality(int32_t B, int32_t NV, int32_t NT, const double* coords, const int32_t* cells, const int32_t* nv,
                                const int32_t* nt, double q_floor, double* qual, int32_t* qinfo, void* stream) {
  if (B <= 0 || NV <= 0 || NT <= 0) return mdq_set_error("mdq_mesh_quality: B, NV and NT must be positive");
  if (!coords || !cells || !nv || !nt || !qual || !qinfo) return mdq_set_error("mdq_mesh_quality: NULL pointer");
  if (((uintptr_t)coords | (uintptr_t)qual | (uintptr_t)qinfo) & 15)
    return mdq_set_error("mdq_mesh_quality: coords, qual and qinfo must be 16-byte aligned");
  if (!(q_floor >= 0.0 && q_floor <= 1.0)) return mdq_set_error("mdq_mesh_quality: q_floor must be finite and lie in [0, 1]");
  hipLaunchKernelGGL(mdq_mesh::mesh_quality_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, NV, NT, coords, cells, nv, nt,
                     q_floor, qual, qinfo);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("mesh_quality_kernel launch failed");
  return 0;
}

extern "C" int mdq_edge_ptr(int32_t B, const int32_t* nedges, int32_t* edge_ptr, void* stream) {
  if (B <= 0 || !nedges || !edge_ptr) return mdq_set_error("mdq_edge_ptr: bad arguments");
  hipLaunchKernelGGL(mdq_mesh::edge_ptr_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, B, nedges, edge_ptr);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("edge_ptr_kernel launch failed");
  return 0;
}
