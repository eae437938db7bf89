// Noisy-network exploration of the device learning loop (Fortunato et al. 2018, factorised Gaussian noise on the dense
// head; no reference counterpart: its exploration is the epsilon-greedy draw of airfoil_dqn.py:452-460) - two launches:
//   pack_noisy_kernel : gcn_pack_kernel (mdq_gcn_train.hip) with up to 4 layers whose packed weights and biases are
//                       mean + sigma * noise; the noise is generated inside the launch (Philox4x32-10, counter-based)
//   noisy_grad_kernel : the sigmas' slices of the flat gradient from the means' slices the learning step wrote
// Semantics: include/meshdqn_hip.h.  No atomics; the same (seed, stream, draw) gives the same bits on every run.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/meshdqn_hip.h"
#include "mdq_internal.h"

namespace mdq_noisy {

constexpr int TILE = 32;    // a weight tile is TILE outputs x TILE inputs, 256 threads = 8 rows of 32 per pass

struct philox_out {
  uint32_t r0, r1;
};

// Philox4x32-10 (Salmon et al. 2011): ten rounds, the key bumped by the Weyl constants between them; the first two of the
// four output words are used
__device__ __forceinline__ philox_out philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {c0, c1};
}

// entry j of side `side` (0 = in, 1 = out) of noisy layer L: f(z) = sign(z) sqrt(|z|) of a Box-Muller normal z.  u1 and
// 2 u2 are exact in float; logf, sqrtf and cospif are the float functions (the header says why cospif).  Products only: there
// is no sum a compiler could contract into, the pragma says so all the same.
__device__ __forceinline__ float noise(const mdq_noisy_desc& Z, int L, int side, int j) {
#pragma clang fp contract(off)
  const philox_out p = philox4x32_10((uint32_t)j, (uint32_t)(2 * L + side), (uint32_t)Z.draw, (uint32_t)(Z.draw >> 32), Z.seed, Z.stream);
  const float u1 = (float)((p.r0 >> 8) + 1u) * 0x1p-24f;
  const float t2 = (float)(p.r1 >> 8) * 0x1p-23f;       // 2 u2
  const float rad = sqrtf(-2.0f * logf(u1));
  const float z = rad * cospif(t2);
  return copysignf(sqrtf(fabsf(z)), z);
}

// The grid of gcn_pack_kernel: blockIdx.y is the table segment, gridDim.x workgroups share it.  A segment no noisy layer
// names: that kernel's loop.  A noisy weight segment: tiles of TILE x TILE - the means and sigmas are read along the input
// index (consecutive in torch's [out][in]), composed, turned in LDS (rows padded by one float: the column reads of the
// store pass hit 32 different banks) and written along the output index (consecutive in the packed [in][out]).  The 2 x TILE
// noise values of a tile are recomputed by the workgroup that owns it; workgroup 0 of the segment stores both vectors.
__global__ __launch_bounds__(256) void pack_noisy_kernel(mdq_gcn_pack_table T, mdq_noisy_desc Z) {
  __shared__ float tile[TILE][TILE + 1];
  __shared__ float e_in[TILE], e_out[TILE];
  const int s = blockIdx.y;
  if (s >= T.n) return;
  const int rows = T.rows[s], cols = T.cols[s];
  const float* __restrict__ src = T.src[s];
  float* __restrict__ dst = T.dst[s];
  int L = -1, bias = 0;
  for (int l = 0; l < Z.n; ++l) {
    if (Z.seg_w[l] == s) L = l;
    if (Z.seg_b[l] == s) L = l, bias = 1;
  }
  if (L < 0) {
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < rows * cols; idx += gridDim.x * 256) {
      const int c = idx / rows, r = idx - c * rows;       // consecutive threads write consecutive dst entries
      dst[idx] = src[(size_t)r * cols + c];
    }
    return;
  }
  if (bias) {
    const float* __restrict__ sb = Z.sigma_b[L];
    for (int o = blockIdx.x * 256 + threadIdx.x; o < rows; o += gridDim.x * 256) {
#pragma clang fp contract(off)
      const float q = sb[o] * noise(Z, L, 1, o);
      dst[o] = src[o] + q;
    }
    return;
  }
  const int out = rows, in = cols;
  if (blockIdx.x == 0) {
    for (int j = threadIdx.x; j < in; j += 256) Z.eps_in[L][j] = noise(Z, L, 0, j);
    for (int j = threadIdx.x; j < out; j += 256) Z.eps_out[L][j] = noise(Z, L, 1, j);
  }
  const float* __restrict__ sw = Z.sigma_w[L];
  const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x >> 5;
  const int tiles_i = (in + TILE - 1) / TILE, tiles_o = (out + TILE - 1) / TILE;
  for (int t = blockIdx.x; t < tiles_i * tiles_o; t += gridDim.x) {      // (the bounds are the workgroup's: barriers are safe)
    const int o0 = (t / tiles_i) * TILE, i0 = (t - (t / tiles_i) * tiles_i) * TILE;
    __syncthreads();                                                     // the previous tile's store pass has read the LDS
    if (ty == 0) e_in[tx] = i0 + tx < in ? noise(Z, L, 0, i0 + tx) : 0.f;
    if (ty == 1) e_out[tx] = o0 + tx < out ? noise(Z, L, 1, o0 + tx) : 0.f;
    __syncthreads();
    for (int r = ty; r < TILE; r += 256 / TILE) {
      const int o = o0 + r, i = i0 + tx;
      if (o < out && i < in) {
#pragma clang fp contract(off)
        const size_t at = (size_t)o * in + i;
        const float p = e_out[r] * e_in[tx];
        const float q = sw[at] * p;
        tile[r][tx] = src[at] + q;
      }
    }
    __syncthreads();
    for (int c = ty; c < TILE; c += 256 / TILE) {
      const int i = i0 + c, o = o0 + tx;
      if (o < out && i < in) dst[(size_t)i * out + o] = tile[tx][c];
    }
  }
}

// blockIdx.y is the layer; one thread per entry of its weight (then bias) slice, the grid of adam_kernel
__global__ __launch_bounds__(256) void noisy_grad_kernel(mdq_noisy_desc Z, mdq_noisy_grad_layout Y, float* __restrict__ grad) {
  const int L = blockIdx.y;
  if (L >= Z.n) return;
  const int out = Y.out[L], in = Y.in[L];
  const float* __restrict__ ei = Z.eps_in[L];
  const float* __restrict__ eo = Z.eps_out[L];
  for (int e = blockIdx.x * 256 + threadIdx.x; e < out * in + out; e += gridDim.x * 256) {
#pragma clang fp contract(off)
    if (e < out * in) {
      const int o = e / in, i = e - o * in;
      const float p = eo[o] * ei[i];
      grad[Y.sig_w[L] + e] = grad[Y.mu_w[L] + e] * p;
    } else {
      const int o = e - out * in;
      grad[Y.sig_b[L] + o] = grad[Y.mu_b[L] + o] * eo[o];
    }
  }
}

static const char* check_desc(const mdq_noisy_desc* nz, bool sigmas) {
  if (!nz) return "nz is NULL";
  if (nz->n < 1 || nz->n > MDQ_NOISY_MAX) return "n outside 1 .. 4";
  for (int l = 0; l < nz->n; ++l) {
    if (sigmas && (!nz->sigma_w[l] || !nz->sigma_b[l])) return "NULL sigma_w or sigma_b";
    if (!nz->eps_in[l] || !nz->eps_out[l]) return "NULL eps_in or eps_out";
  }
  return nullptr;
}

}  // namespace mdq_noisy

extern "C" int mdq_gcn_pack_noisy(const mdq_gcn_pack_table* table, const mdq_noisy_desc* nz, void* stream) {
  using namespace mdq_noisy;
  if (!table || table->n <= 0 || table->n > MDQ_GCN_PACK_MAX) return mdq_set_error("mdq_gcn_pack_noisy: bad table (n outside 1 .. 32)");
  if (const char* why = check_desc(nz, true)) return mdq_set_error((std::string("mdq_gcn_pack_noisy: ") + why).c_str());
  bool named[MDQ_GCN_PACK_MAX] = {};
  for (int l = 0; l < nz->n; ++l) {
    const int w = nz->seg_w[l], b = nz->seg_b[l];
    if (w < 0 || w >= table->n || b < 0 || b >= table->n) return mdq_set_error("mdq_gcn_pack_noisy: seg_w or seg_b outside the table");
    if (w == b || named[w] || named[b]) return mdq_set_error("mdq_gcn_pack_noisy: seg_w / seg_b name a segment twice");
    named[w] = named[b] = true;
    if (table->rows[w] < 1 || table->cols[w] < 1) return mdq_set_error("mdq_gcn_pack_noisy: weight segment (seg_w) with rows or cols < 1");
    if (table->rows[b] != table->rows[w] || table->cols[b] != 1)
      return mdq_set_error("mdq_gcn_pack_noisy: bias segment (seg_b) must have the weight segment's rows and cols 1");
  }
  hipLaunchKernelGGL(pack_noisy_kernel, dim3(16, table->n), dim3(256), 0, (hipStream_t)stream, *table, *nz);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("mdq_gcn_pack_noisy: pack_noisy_kernel launch failed");
  return 0;
}

extern "C" int mdq_noisy_grad(const mdq_noisy_desc* nz, const mdq_noisy_grad_layout* lay, float* grad, void* stream) {
  using namespace mdq_noisy;
  if (const char* why = check_desc(nz, false)) return mdq_set_error((std::string("mdq_noisy_grad: ") + why).c_str());
  if (!lay || !grad) return mdq_set_error("mdq_noisy_grad: lay or grad is NULL");
  int64_t lo[4 * MDQ_NOISY_MAX], hi[4 * MDQ_NOISY_MAX];
  int m = 0;
  for (int l = 0; l < nz->n; ++l) {
    const int64_t out = lay->out[l], in = lay->in[l];
    if (out < 1 || in < 1) return mdq_set_error("mdq_noisy_grad: out or in < 1");
    const int64_t off[4] = {lay->mu_w[l], lay->mu_b[l], lay->sig_w[l], lay->sig_b[l]};
    const int64_t len[4] = {out * in, out, out * in, out};
    for (int k = 0; k < 4; ++k, ++m) {
      lo[m] = off[k], hi[m] = off[k] + len[k];
      if (lo[m] < 0 || hi[m] > (int64_t)lay->total)
        return mdq_set_error("mdq_noisy_grad: a slice (mu_w, mu_b, sig_w, sig_b) outside [0, total)");
    }
  }
  for (int a = 0; a < m; ++a)
    for (int b = a + 1; b < m; ++b)
      if (lo[a] < hi[b] && lo[b] < hi[a]) return mdq_set_error("mdq_noisy_grad: slices (mu_w, mu_b, sig_w, sig_b) overlap");
  hipLaunchKernelGGL(noisy_grad_kernel, dim3(16, nz->n), dim3(256), 0, (hipStream_t)stream, *nz, *lay, grad);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("mdq_noisy_grad: noisy_grad_kernel launch failed");
  return 0;
}
