// Target network of the device learning loop (no reference counterpart: its two networks swap roles and never exchange
// weights, airfoil_dqn.py:184-200,240-310) - two small launches of the optimiser chain around the unchanged learning step:
//   double_q_select_kernel : Double DQN (van Hasselt et al. 2016): per row the first maximum of the ONLINE network's outputs
//                            picks the entry of the TARGET network's outputs; the row handed on holds that value in every
//                            column, so the mode-0 `max_j q_other[b][j]` of gcn_train_kernel returns exactly it
//   target_update_kernel   : the target's parameters follow the online ones: a copy of the bits (tau = 1, Mnih et al. 2015)
//                            or Polyak averaging, every parameter tensor in one launch
// Semantics: include/meshdqn_hip.h.  No atomics, no LDS, no device random numbers: run-to-run identical.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/meshdqn_hip.h"
#include "mdq_internal.h"

namespace mdq_target {

constexpr int ROWS = MDQ_DOUBLE_Q_ROWS;   // rows (= waves) per workgroup

// One wave per row.  Lane l walks the columns l, l + 64, ...: a strict `>` keeps the first maximum of its own columns and
// never takes a NaN; the butterfly then keeps, of two lanes' pairs, the larger value and among equal values (-0 == +0) the
// smaller column.  That order is total on the pairs a row can hold, so all 64 lanes end with the same pair.  A lane without
// a candidate carries (-inf, INT_MAX), which loses against every candidate; nothing above -inf in the whole row: column 0.
__global__ __launch_bounds__(64 * ROWS) void double_q_select_kernel(int B, int OUT, const float* __restrict__ q_online,
                                                                    const float* __restrict__ q_target, float* q_sel,
                                                                    int32_t* sel) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * ROWS + (threadIdx.x >> 6);
  if (b >= B) return;   // (a whole wave: the shuffles below never straddle rows)
  const size_t row = (size_t)b * (size_t)OUT;
  float best = -INFINITY;
  int bj = INT_MAX;
  for (int j = lane; j < OUT; j += 64) {
    const float q = q_online[row + j];
    if (q > best) {
      best = q;
      bj = j;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oj = __shfl_xor(bj, off, 64);
    if (ov > best || (ov == best && oj < bj)) {
      best = ov;
      bj = oj;
    }
  }
  const int js = bj == INT_MAX ? 0 : bj;
  const float v = q_target[row + js];
  for (int c = lane; c < OUT; c += 64) q_sel[row + c] = v;
  if (sel && lane == 0) sel[b] = js;
}

// One thread per parameter element of every tensor, the grid of adam_kernel.  The values travel as 32-bit words: tau = 1
// hands on src's bits whatever they encode; otherwise dst + tf * (src - dst) in three float operations, each rounded on
// its own (contraction is switched off for the block: the intrinsics alone do not keep the compiler from forming an fma).
__global__ __launch_bounds__(256) void target_update_kernel(mdq_target_update_desc D) {
  const int s = blockIdx.y;
  if (s >= D.n) return;
  uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(D.dst[s]);
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(D.src[s]);
  const int len = D.len[s];
  const bool copy = D.tau == 1.0;
  const float tf = (float)D.tau;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < len; i += gridDim.x * 256) {
    const uint32_t sw = src[i];
    if (copy) {
      dst[i] = sw;
    } else {
#pragma clang fp contract(off)
      const float d = __uint_as_float(dst[i]), sv = __uint_as_float(sw);
      const float diff = sv - d;
      const float step = tf * diff;
      const float r = d + step;
      dst[i] = __float_as_uint(r);
    }
  }
}

}  // namespace mdq_target

extern "C" int mdq_double_q_select(int32_t B, int32_t OUT, const float* q_online, const float* q_target, float* q_sel,
                                   int32_t* sel, void* stream) {
  if (B <= 0 || OUT <= 0) return mdq_set_error("mdq_double_q_select: B and OUT must be positive");
  if (!q_online || !q_target || !q_sel) return mdq_set_error("mdq_double_q_select: q_online, q_target and q_sel must not be NULL");
  const uintptr_t bytes = (uintptr_t)B * (uintptr_t)OUT * sizeof(float), o = (uintptr_t)q_sel;
  for (const float* in : {q_online, q_target}) {
    const uintptr_t a = (uintptr_t)in;
    if (o < a + bytes && a < o + bytes) return mdq_set_error("mdq_double_q_select: q_sel overlaps an input");
  }
  hipLaunchKernelGGL(mdq_target::double_q_select_kernel, dim3((unsigned)((B + mdq_target::ROWS - 1) / mdq_target::ROWS)),
                     dim3(64 * mdq_target::ROWS), 0, (hipStream_t)stream, B, OUT, q_online, q_target, q_sel, sel);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("mdq_double_q_select: double_q_select_kernel launch failed");
  return 0;
}

extern "C" int mdq_target_update(const mdq_target_update_desc* d, void* stream) {
  if (!d || d->n < 1 || d->n > MDQ_GCN_PACK_MAX) return mdq_set_error("mdq_target_update: n outside 1 .. 32");
  if (!std::isfinite(d->tau) || !(d->tau > 0.0) || d->tau > 1.0) return mdq_set_error("mdq_target_update: tau must lie in (0, 1]");
  for (int s = 0; s < d->n; ++s) {
    if (!d->dst[s] || !d->src[s]) return mdq_set_error("mdq_target_update: NULL tensor");
    if (d->len[s] < 0) return mdq_set_error("mdq_target_update: negative len");
    if (d->dst[s] == d->src[s]) return mdq_set_error("mdq_target_update: dst equals src");
  }
  hipLaunchKernelGGL(mdq_target::target_update_kernel, dim3(32, d->n), dim3(256), 0, (hipStream_t)stream, *d);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("mdq_target_update: target_update_kernel launch failed");
  return 0;
}
