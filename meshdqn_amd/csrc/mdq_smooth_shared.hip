// What the smoothing kernels of mdq_smooth.hip, mdq_smooth_linear.hip and mdq_smooth_big.hip share: the 8-lane reductions,
// the Newton reciprocals, the block scan, the sweep count and DOLFIN's exact update.  A fragment (every function is inlined
// into the kernel that calls it: no symbol of its own), included by each of the three files.  The kernels' machine code is
// held byte for byte across edits of this text (tools/same_device_code.py): smooth_linear_kernel, the dominant kernel of the
// env step, keeps a few of these written out where the shared function moved its code - the places say so.
#pragma once
#include <hip/hip_runtime.h>

namespace mdq_smooth_shared {
typedef double d2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// all-reduce over groups of 8 consecutive lanes: xor 1, xor 2 (quad_perm), then the other quad (row_half_mirror)
__device__ __forceinline__ double grp8_sum(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  return v;
}
__device__ __forceinline__ double grp8_min(double v) {
  v = fmin(v, dpp_f64<0xB1>(v));
  v = fmin(v, dpp_f64<0x4E>(v));
  v = fmin(v, dpp_f64<0x141>(v));
  return v;
}
// 1/sqrt(x) and 1/x to double precision (~1 ulp): hardware estimate + two Newton steps (exact update only)
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
  y = y * (1.5 - h * y * y);
  y = y * (1.5 - h * y * y);
  return y;
}
__device__ __forceinline__ double rcp_nr(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = y * (2.0 - x * y);
  y = y * (2.0 - x * y);
  return y;
}

// sweeps of environment b: given per environment, or - inside an env step - `iters_env` where a vertex was removed
// successfully (Env2DAirfoil._check_mesh -> flow_solver.remesh -> smooth(50), flow_solver.py:236-237; nothing otherwise)
__device__ __forceinline__ int sweeps_of(int b, const int32_t* iters_, const int32_t* rem, const int32_t* rstat, int iters_env) {
  return iters_ ? iters_[b] : ((rem[b] >= 0 && rstat[b] == 0) ? iters_env : 0);
}

// inclusive scan of data[0..N) in place: the first THREADS threads, N / THREADS consecutive entries each; part = THREADS
// ints of scratch.  A larger workgroup reaches the barriers with all its threads
template <int THREADS, int N>
__device__ __forceinline__ void scan_inclusive(int* data, int* part) {
  constexpr int PER = N / THREADS;
  const int tid = threadIdx.x;
  const bool act = tid < THREADS;
  int loc[PER], run = 0;
  if (act) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      run += data[tid * PER + i];
      loc[i] = run;
    }
    part[tid] = run;
  }
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {   // (Hillis-Steele over the thread totals)
    const int add = (act && tid >= off) ? part[tid - off] : 0;
    __syncthreads();
    if (act) part[tid] += add;
    __syncthreads();
  }
  if (act) {
    const int base = part[tid] - run;
#pragma unroll
    for (int i = 0; i < PER; ++i) data[tid * PER + i] = base + loc[i];
  }
  __syncthreads();
}

// DOLFIN's exact fp64 update of a vertex at p with k incident cells, in two parts.  exact_gather, by the 8 lanes of a
// group (lane l takes the cells l, l + 8, ... of the vertex's ascending-cell list; fetch(q, pa, pc) gives the positions of
// the two other vertices of cell q): the sums of the neighbours' positions (every neighbour appears in two cells) and rm,
// the smallest SQUARED distance from p to the lines through the opposite edges, in all 8 lanes - fixed summation order,
// no contraction: every parity test rests on these bits.  exact_step: the vertex stays when it is closer than DOLFIN_EPS
// to the centroid c, goes to c when |c - p| <= r_min / 2 and r_min / 2 towards it otherwise; r2k = 1 / (2 k)
struct ExactSums { double sx, sy, rm; };
template <class Fetch>
__device__ __forceinline__ ExactSums exact_gather(const d2 p, int k, int l, Fetch fetch) {
#pragma clang fp contract(off)
  double sx = 0.0, sy = 0.0, rm = 1e300;
  for (int q = l; q < k; q += 8) {
    d2 pa, pc;
    fetch(q, pa, pc);
    sx += pa.x + pc.x;
    sy += pa.y + pc.y;
    const double tx = pc.x - pa.x, ty = pc.y - pa.y;
    const double cr = ty * (p.x - pa.x) - tx * (p.y - pa.y);
    rm = fmin(rm, cr * cr * rcp_nr(tx * tx + ty * ty));
  }
  return ExactSums{grp8_sum(sx), grp8_sum(sy), grp8_min(rm)};
}
__device__ __forceinline__ d2 exact_step(const d2 p, double sx, double sy, double rm, double r2k) {
#pragma clang fp contract(off)
  const double EPS = 3.0e-16;
  const double dx = sx * r2k - p.x, dy = sy * r2k - p.y;
  const double q2 = dx * dx + dy * dy;
  if (!(q2 >= EPS * EPS && q2 > 0.0)) return p;          // |c - p| < DOLFIN_EPS: the vertex stays
  if (0.25 * rm < q2) {                                  // limited step: needs the lengths
    const double f = 0.5 * (rm * rsqrt_nr(rm)) * rsqrt_nr(q2);
    return d2{p.x + f * dx, p.y + f * dy};
  }
  return d2{p.x + dx, p.y + dy};                         // |c - p| <= r_min / 2: to the centroid itself
}
}  // namespace mdq_smooth_shared
