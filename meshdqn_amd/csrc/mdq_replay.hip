// Device-resident replay memory and optimiser update of the DQN learning loop: with these kernels a training
// step needs no host round trip and no per-transition Python object -
//   replay_step_kernel   : the B transitions of one batched env step into the record ring
//                          (ReplayMemory.push, airfoil_dqn.py:56-61, for B environments at once)
//   replay_sample_kernel : a minibatch of records -> the arrays of mdq_gcn_forward / mdq_gcn_train_step
//                          (ReplayMemory.sample + the Batch.from_data_list of DataWorker._get_data, airfoil_dqn.py:63-64,240-262)
//   replay_sample_nstep_kernel : the same launch with the n-step transition of every draw composed from the ring's
//                          groups (no reference counterpart: its targets are 1-step)
//   adam_kernel          : torch.optim.Adam.step (weight decay as L2 term, bias corrections) on every trained
//                          parameter in one launch (ParameterServer.apply_gradients, airfoil_dqn.py:184-200)
//   prio_*_kernel        : proportional prioritized replay on the ring (no reference counterpart: its replay is uniform)
// Record layout (float32, the layout of trainer.pack_transitions: what the ranks all-gather when the replay is shared):
//   [ x(s) N*F | x(s') N*F | src(s) EM | dst(s) EM | src(s') EM | dst(s') EM | edges(s) | edges(s') | action | reward | done ]
// (a terminal transition has zeros for s').
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/meshdqn_hip.h"
#include "mdq_internal.h"

namespace mdq_replay {

__global__ __launch_bounds__(256) void replay_step_kernel(float* R, int rec_len, int capacity, int nf, int EM, const float* x,
                                                           const int32_t* es, const int32_t* ed, const int32_t* nedges,
                                                           int base_cur, int base_prev, const int32_t* act,
                                                           const double* rew, const uint8_t* done) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* xb = x + (size_t)b * nf;
  const int32_t* sb = es + (size_t)b * EM;
  const int32_t* db = ed + (size_t)b * EM;
  const int cnt = nedges[b];
  if (base_cur >= 0) {   // the state the next transition of environment b starts from
    float* r = R + (size_t)((base_cur + b) % capacity) * rec_len;
    for (int i = tid; i < nf; i += 256) r[i] = xb[i];
    for (int e = tid; e < EM; e += 256) {
      r[2 * nf + e] = e < cnt ? (float)sb[e] : 0.f;
      r[2 * nf + EM + e] = e < cnt ? (float)db[e] : 0.f;
    }
    if (tid == 0) r[2 * nf + 4 * EM] = (float)cnt;
  }
  if (base_prev >= 0) {  // ... and the state the previous one ended in (nothing if that one was terminal: the
    float* r = R + (size_t)((base_prev + b) % capacity) * rec_len;   // environment has been reset in place since)
    const bool dn = done[b] != 0;
    for (int i = tid; i < nf; i += 256) r[nf + i] = dn ? 0.f : xb[i];
    for (int e = tid; e < EM; e += 256) {
      const bool live = !dn && e < cnt;
      r[2 * nf + 2 * EM + e] = live ? (float)sb[e] : 0.f;
      r[2 * nf + 3 * EM + e] = live ? (float)db[e] : 0.f;
    }
    if (tid == 0) {
      float* t = r + 2 * nf + 4 * EM;
      t[1] = dn ? 0.f : (float)cnt;
      t[2] = (float)act[b];
      t[3] = (float)rew[b];
      t[4] = dn ? 1.f : 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void replay_sample_kernel(mdq_replay_sample_desc D) {
  const int i = blockIdx.x, tid = threadIdx.x, nf = D.nf, EM = D.EM, tail = 2 * nf + 4 * EM;
  __shared__ int red[2][256];
  // packed edge offsets of this transition's two graphs: counts of the transitions before it
  int c0 = 0, c1 = 0;
  for (int j = tid; j < i; j += 256) {
    const float* t = D.R + (size_t)D.idx[j] * D.rec_len + tail;
    c0 += (int)t[0];
    c1 += t[4] > 0.5f ? (int)t[0] : (int)t[1];     // terminal: its own state as a masked placeholder
  }
  red[0][tid] = c0;
  red[1][tid] = c1;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
    }
    __syncthreads();
  }
  const int o0 = red[0][0], o1 = red[1][0];
  const float* r = D.R + (size_t)D.idx[i] * D.rec_len;
  const float* t = r + tail;
  const bool dn = t[4] > 0.5f;
  const int n0 = (int)t[0], n1 = dn ? n0 : (int)t[1];
  const float* xn = dn ? r : r + nf;
  const float* sn = dn ? r + 2 * nf : r + 2 * nf + 2 * EM;
  for (int k = tid; k < nf; k += 256) {
    D.x_s[(size_t)i * nf + k] = r[k];
    D.x_n[(size_t)i * nf + k] = xn[k];
  }
  for (int e = tid; e < n0; e += 256) {
    D.esrc_s[o0 + e] = (int32_t)r[2 * nf + e];
    D.edst_s[o0 + e] = (int32_t)r[2 * nf + EM + e];
  }
  for (int e = tid; e < n1; e += 256) {
    D.esrc_n[o1 + e] = (int32_t)sn[e];
    D.edst_n[o1 + e] = (int32_t)sn[EM + e];
  }
  if (tid == 0) {
    D.edge_ptr_s[i] = o0;
    D.edge_ptr_n[i] = o1;
    if (i == (int)gridDim.x - 1) {
      D.edge_ptr_s[i + 1] = o0 + n0;
      D.edge_ptr_n[i + 1] = o1 + n1;
    }
    D.action[i] = (int64_t)t[2];
    D.reward[i] = t[3];
    D.nonfinal[i] = dn ? 0.f : 1.f;
  }
}

// The last record of the n-step walk from record j0 (semantics: include/meshdqn_hip.h): successor (j + W) % capacity, at most
// n_step records, never past a terminal one and never INTO the group at `head`.  A chain of dependent reads of `done`.
__device__ __forceinline__ int nstep_last(const float* R, int rec_len, int tail, const mdq_replay_nstep& S, int j0) {
  int j = j0;
  for (int k = 1; k < S.n_step; ++k) {
    if (R[(size_t)j * rec_len + tail + 4] > 0.5f) break;
    const int nx = (int)(((unsigned)j + (unsigned)S.W) % (unsigned)S.capacity);
    if (nx >= S.head && nx < S.head + S.W) break;
    j = nx;
  }
  return j;
}

// replay_sample_kernel with the n-step transition of every draw composed on the way: s, its edges and the action of
// record idx[i]; s' and its edges of the walk's last record; the discounted reward sum and gamma^(m-1) in `nonfinal`.
__global__ __launch_bounds__(256) void replay_sample_nstep_kernel(mdq_replay_sample_desc D, mdq_replay_nstep S) {
  const int i = blockIdx.x, tid = threadIdx.x, nf = D.nf, EM = D.EM, tail = 2 * nf + 4 * EM;
  __shared__ int red[2][256];
  __shared__ int own[2];      // last record of this draw's walk, records taken
  __shared__ float ownf[2];   // reward, nonfinal
  // packed edge offsets of this transition's two graphs: counts of the transitions before it, each behind its own walk
  int c0 = 0, c1 = 0;
  for (int j = tid; j < i; j += 256) {
    const int j0 = D.idx[j];
    const float* t0 = D.R + (size_t)j0 * D.rec_len + tail;
    const float* tl = D.R + (size_t)nstep_last(D.R, D.rec_len, tail, S, j0) * D.rec_len + tail;
    c0 += (int)t0[0];
    c1 += tl[4] > 0.5f ? (int)t0[0] : (int)tl[1];   // terminal: the own state of idx[j] as a masked placeholder
  }
  red[0][tid] = c0;
  red[1][tid] = c1;
  if (tid == 0) {   // this draw's own walk, once: fp64, every product and every sum rounded on its own, in the order of k
#pragma clang fp contract(off)   // (plain operators under this pragma: HIP's __dmul_rn / __dadd_rn do not stop an fma)
    int j = D.idx[i], m = 1;
    const float* t = D.R + (size_t)j * D.rec_len + tail;
    double g = 1.0, acc = (double)t[3];
    while (m < S.n_step && !(t[4] > 0.5f)) {
      const int nx = (int)(((unsigned)j + (unsigned)S.W) % (unsigned)S.capacity);
      if (nx >= S.head && nx < S.head + S.W) break;
      j = nx;
      t = D.R + (size_t)j * D.rec_len + tail;
      g = g * S.gamma;
      const double term = g * (double)t[3];
      acc = acc + term;
      ++m;
    }
    own[0] = j;
    own[1] = m;
    ownf[0] = (float)acc;
    ownf[1] = t[4] > 0.5f ? 0.f : (float)g;   // gamma^(m-1): the learning step multiplies by (float)gamma once more
  }
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      red[0][tid] += red[0][tid + off];
      red[1][tid] += red[1][tid + off];
    }
    __syncthreads();
  }
  const int o0 = red[0][0], o1 = red[1][0];
  const float* r = D.R + (size_t)D.idx[i] * D.rec_len;
  const float* rl = D.R + (size_t)own[0] * D.rec_len;
  const float* t = r + tail;
  const bool dn = rl[tail + 4] > 0.5f;
  const int n0 = (int)t[0], n1 = dn ? n0 : (int)rl[tail + 1];
  const float* xn = dn ? r : rl + nf;
  const float* sn = dn ? r + 2 * nf : rl + 2 * nf + 2 * EM;
  for (int k = tid; k < nf; k += 256) {
    D.x_s[(size_t)i * nf + k] = r[k];
    D.x_n[(size_t)i * nf + k] = xn[k];
  }
  for (int e = tid; e < n0; e += 256) {
    D.esrc_s[o0 + e] = (int32_t)r[2 * nf + e];
    D.edst_s[o0 + e] = (int32_t)r[2 * nf + EM + e];
  }
  for (int e = tid; e < n1; e += 256) {
    D.esrc_n[o1 + e] = (int32_t)sn[e];
    D.edst_n[o1 + e] = (int32_t)sn[EM + e];
  }
  if (tid == 0) {
    D.edge_ptr_s[i] = o0;
    D.edge_ptr_n[i] = o1;
    if (i == (int)gridDim.x - 1) {
      D.edge_ptr_s[i + 1] = o0 + n0;
      D.edge_ptr_n[i + 1] = o1 + n1;
    }
    D.action[i] = (int64_t)t[2];
    D.reward[i] = ownf[0];
    D.nonfinal[i] = ownf[1];
    if (S.steps) S.steps[i] = own[1];
  }
}

// torch.optim.Adam (amsgrad False, maximize False), one thread per parameter element of every segment
__global__ __launch_bounds__(256) void adam_kernel(mdq_adam_desc D) {
  const int s = blockIdx.y;
  if (s >= D.n) return;
  float* p = D.param[s];
  const int len = D.len[s], off = D.offset[s];
  const float lr_c = (float)(D.lr / D.bias_correction1), bc2s = (float)sqrt(D.bias_correction2);
  const float b2 = (float)D.beta2, eps = (float)D.eps, wd = (float)D.weight_decay;
  // the weights as torch forms them: 1 - beta in double, rounded once (1.f - (float)beta2 is off by 1.3e-5 of itself)
  const float w1 = (float)(1.0 - D.beta1), w2 = (float)(1.0 - D.beta2);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < len; i += gridDim.x * 256) {
    float g = D.grad[off + i];
    const float w = p[i];
    if (wd != 0.f) g = fmaf(wd, w, g);
    const float m = D.exp_avg[off + i] + w1 * (g - D.exp_avg[off + i]);      // lerp, as torch does
    const float v = b2 * D.exp_avg_sq[off + i] + w2 * (g * g);
    D.exp_avg[off + i] = m;
    D.exp_avg_sq[off + i] = v;
    p[i] = w - lr_c * (m / (sqrtf(v) / bc2s + eps));
  }
}

}  // namespace mdq_replay

extern "C" int mdq_replay_step(float* ring, int32_t rec_len, int32_t capacity, int32_t B, int32_t nf, int32_t EM,
                               const float* x, const int32_t* edge_src, const int32_t* edge_dst, const int32_t* nedges,
                               int32_t base_cur, int32_t base_prev, const int32_t* action, const double* reward,
                               const uint8_t* done, void* stream) {
  if (!ring || B <= 0 || !x || !edge_src || !edge_dst || !nedges || rec_len != 2 * nf + 4 * EM + 5 || capacity <= 0 ||
      (base_prev >= 0 && (!action || !reward || !done)))
    return mdq_set_error("mdq_replay_step: bad arguments");
  hipLaunchKernelGGL(mdq_replay::replay_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, ring, rec_len, capacity, nf,
                     EM, x, edge_src, edge_dst, nedges, base_cur, base_prev, action, reward, done);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("replay_step_kernel launch failed");
  return 0;
}

extern "C" int mdq_replay_sample_nstep(const mdq_replay_sample_desc* d, const mdq_replay_nstep* ns, void* stream) {
  if (!d || d->n <= 0 || !d->R || !d->idx || d->rec_len != 2 * d->nf + 4 * d->EM + 5 || !d->x_s || !d->x_n || !d->esrc_s ||
      !d->edst_s || !d->esrc_n || !d->edst_n || !d->edge_ptr_s || !d->edge_ptr_n || !d->action || !d->reward || !d->nonfinal)
    return mdq_set_error(ns ? "mdq_replay_sample_nstep: bad arguments" : "mdq_replay_sample: bad arguments");
  if (!ns) {
    hipLaunchKernelGGL(mdq_replay::replay_sample_kernel, dim3(d->n), dim3(256), 0, (hipStream_t)stream, *d);
    if (hipGetLastError() != hipSuccess) return mdq_set_error("replay_sample_kernel launch failed");
    return 0;
  }
  if (ns->n_step < 1 || ns->n_step > 64) return mdq_set_error("mdq_replay_sample_nstep: n_step outside 1 .. 64");
  if (ns->W < 1) return mdq_set_error("mdq_replay_sample_nstep: W must be positive");
  if (ns->capacity < 2 * (long long)ns->W || ns->capacity % ns->W != 0)
    return mdq_set_error("mdq_replay_sample_nstep: capacity must be a multiple of W and at least 2 W");
  if (ns->head < 0 || ns->head >= ns->capacity || ns->head % ns->W != 0)
    return mdq_set_error("mdq_replay_sample_nstep: head must be a multiple of W in [0, capacity)");
  if (!(ns->gamma >= 0.0) || !std::isfinite(ns->gamma))
    return mdq_set_error("mdq_replay_sample_nstep: gamma must be finite and not negative");
  hipLaunchKernelGGL(mdq_replay::replay_sample_nstep_kernel, dim3(d->n), dim3(256), 0, (hipStream_t)stream, *d, *ns);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("replay_sample_nstep_kernel launch failed");
  return 0;
}

extern "C" int mdq_replay_sample(const mdq_replay_sample_desc* d, void* stream) { return mdq_replay_sample_nstep(d, nullptr, stream); }

extern "C" int mdq_adam_step(const mdq_adam_desc* d, void* stream) {
  if (!d) return mdq_set_error("mdq_adam_step: NULL descriptor");
  if (d->n < 1 || d->n > MDQ_GCN_PACK_MAX) return mdq_set_error("mdq_adam_step: n outside 1 .. 32");
  if (!d->grad) return mdq_set_error("mdq_adam_step: grad is NULL");
  if (!d->exp_avg) return mdq_set_error("mdq_adam_step: exp_avg is NULL");
  if (!d->exp_avg_sq) return mdq_set_error("mdq_adam_step: exp_avg_sq is NULL");
  for (int s = 0; s < d->n; ++s) {
    if (d->len[s] < 0) return mdq_set_error("mdq_adam_step: negative len");
    if (d->offset[s] < 0) return mdq_set_error("mdq_adam_step: negative offset");
    if ((long long)d->offset[s] + d->len[s] > INT32_MAX) return mdq_set_error("mdq_adam_step: offset + len beyond int32");
    if (d->len[s] > 0 && !d->param[s]) return mdq_set_error("mdq_adam_step: param is NULL where len > 0");
  }
  if (!std::isfinite(d->lr) || d->lr < 0.0) return mdq_set_error("mdq_adam_step: lr must be finite and not negative");
  if (!std::isfinite(d->eps) || d->eps < 0.0) return mdq_set_error("mdq_adam_step: eps must be finite and not negative");
  if (!std::isfinite(d->weight_decay) || d->weight_decay < 0.0)
    return mdq_set_error("mdq_adam_step: weight_decay must be finite and not negative");
  if (!(d->beta1 >= 0.0 && d->beta1 < 1.0)) return mdq_set_error("mdq_adam_step: beta1 outside [0, 1)");
  if (!(d->beta2 >= 0.0 && d->beta2 < 1.0)) return mdq_set_error("mdq_adam_step: beta2 outside [0, 1)");
  if (!(d->bias_correction1 > 0.0 && d->bias_correction1 <= 1.0))
    return mdq_set_error("mdq_adam_step: bias_correction1 outside (0, 1]");
  if (!(d->bias_correction2 > 0.0 && d->bias_correction2 <= 1.0))
    return mdq_set_error("mdq_adam_step: bias_correction2 outside (0, 1]");
  hipLaunchKernelGGL(mdq_replay::adam_kernel, dim3(32, d->n), dim3(256), 0, (hipStream_t)stream, *d);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("adam_kernel launch failed");
  return 0;
}

// ---------------------------------------------------------------- proportional prioritized replay
// prio[capacity] holds (|td| + eps)^alpha of every record, 0 for a record that must not be sampled (never written, or of
// the group being written).  Three kernels on the optimiser stream (semantics: include/meshdqn_hip.h):
//   prio_fill_kernel   : a finished group gets the largest priority seen so far, the group about to be written gets 0
//   prio_draw_kernel   : one workgroup: fp64 prefix sums of prio, stratified draw of n records, importance weights
//   prio_update_kernel : one workgroup: new priorities of the drawn records from their TD errors
namespace mdq_replay {

constexpr int PT = 1024;   // threads of the draw's workgroup = segments of the priority array

__global__ __launch_bounds__(256) void prio_fill_kernel(float* prio, int capacity, int base_new, int n_new, int base_zero,
                                                        int n_zero, const float* pmax) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_new)
    prio[(int)(((long long)base_new + i) % capacity)] = *pmax;
  else if (i - n_new < n_zero)
    prio[(int)(((long long)base_zero + (i - n_new)) % capacity)] = 0.f;
}

// segment k of the 1024 in a table padded by one slot per 32: the 32 threads that walk 32 consecutive segments each
// hit 32 different LDS banks
__device__ __forceinline__ int pslot(int k) { return k + (k >> 5); }

__global__ __launch_bounds__(PT) void prio_draw_kernel(mdq_replay_prio_draw_desc D) {
  __shared__ double seg[PT + PT / 32];   // sum of every segment; then E[k]: sum of everything in front of segment k
  __shared__ double grp[32];
  __shared__ double total_s;
  __shared__ int lastpos[PT];
  __shared__ float pmin[PT];
  const int tid = threadIdx.x, cap = D.capacity, n = D.n;
  const float* __restrict__ prio = D.prio;
  // segment k = records [k L, (k + 1) L): the order of every sum below is a function of the capacity alone
  const long long L = ((long long)cap + PT - 1) / PT;
  {
    const int j0 = (int)min(tid * L, (long long)cap), j1 = (int)min((tid + 1) * L, (long long)cap);
    double s = 0.0;
    int lp = -1;
    for (int j = j0; j < j1; ++j) {
      const float p = prio[j];
      s += (double)p;
      if (p > 0.f) lp = j;
    }
    seg[pslot(tid)] = s;
    lastpos[tid] = lp;
  }
  __syncthreads();
  if (tid < 32) {   // 32 groups of 32 segments, every sum serial in index order
    double g = 0.0;
    for (int m = 0; m < 32; ++m) g += seg[pslot(tid * 32 + m)];
    grp[tid] = g;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0;
    for (int g = 0; g < 32; ++g) {
      const double v = grp[g];
      grp[g] = a;
      a += v;
    }
    total_s = a;
  }
  __syncthreads();
  if (tid < 32) {
    const double G = grp[tid];
    double part = 0.0;
    for (int m = 0; m < 32; ++m) {
      const int sl = pslot(tid * 32 + m);
      const double v = seg[sl];
      seg[sl] = G + part;   // non-decreasing in k: sums of non-negative terms, each rounded monotonically
      part += v;
    }
  }
  for (int off = PT / 2; off > 0; off >>= 1) {   // the last record with a priority
    __syncthreads();
    if (tid < off) lastpos[tid] = max(lastpos[tid], lastpos[tid + off]);
  }
  __syncthreads();
  const double total = total_s;
  const bool live = tid < n && total > 0.0;
  int my = 0;
  float pv = 0.f;
  if (live) {
    const double t = total * (((double)tid + D.u[tid]) / (double)n);
    int lo = 0, hi = PT - 1;   // the last segment that starts at or below t (E[0] = 0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (seg[pslot(mid)] <= t)
        lo = mid;
      else
        hi = mid - 1;
    }
    // inclusive prefix of record j of segment k = E[k] + (sum of the segment up to j); the walk goes on into the next
    // segments where rounding left every prefix of this one at or below t
    int found = -1;
    for (int k = lo; k < PT && found < 0; ++k) {
      const long long a0 = k * L;
      if (a0 >= cap) break;
      const int j1 = (int)min(a0 + L, (long long)cap);
      const double E = seg[pslot(k)];
      double loc = 0.0;
      for (int j = (int)a0; j < j1; ++j) {
        const float p = prio[j];
        loc += (double)p;
        if (p > 0.f && E + loc > t) {
          found = j;
          break;
        }
      }
    }
    my = found >= 0 ? found : lastpos[0];   // (i + u) / n rounded to 1: the last record with a priority
    pv = prio[my];
  }
  pmin[tid] = live ? pv : INFINITY;
  for (int off = PT / 2; off > 0; off >>= 1) {
    __syncthreads();
    if (tid < off) pmin[tid] = fminf(pmin[tid], pmin[tid + off]);
  }
  __syncthreads();
  if (tid < n) {
    D.idx[tid] = my;
    D.weight[tid] = live ? (float)pow((double)pmin[0] / (double)pv, D.beta) : 0.f;
  }
  if (tid == 0 && D.total) D.total[0] = total;
}

__global__ __launch_bounds__(PT) void prio_update_kernel(float* prio, int capacity, int n, const int32_t* idx, const float* td,
                                                          double alpha, double eps, float* pmax) {
  __shared__ int sidx[PT];
  __shared__ float sval[PT];
  const int tid = threadIdx.x;
  int id = -1;      // < 0: nothing to write (no draw i, record number out of range, TD error not finite)
  float v = 0.f;
  if (tid < n) {
    const int j = idx[tid];
    const float d = td[tid];
    if (j >= 0 && j < capacity && isfinite(d)) {
      id = j;
      v = (float)pow(fabs((double)d) + eps, alpha);
    }
  }
  sidx[tid] = id;
  sval[tid] = v;
  __syncthreads();
  bool win = id >= 0;   // among the draws of one record the last one writes
  for (int k = tid + 1; k < n && win; ++k) win = sidx[k] != id;
  if (win) prio[id] = v;
  for (int off = blockDim.x / 2; off > 0; off >>= 1) {
    __syncthreads();
    if (tid < off) sval[tid] = fmaxf(sval[tid], sval[tid + off]);
  }
  if (tid == 0) *pmax = fmaxf(*pmax, sval[0]);
}

}  // namespace mdq_replay

extern "C" int mdq_replay_prio_fill(float* prio, int32_t capacity, int32_t base_new, int32_t n_new, int32_t base_zero,
                                    int32_t n_zero, const float* pmax, void* stream) {
  if (!prio || !pmax || capacity <= 0 || n_new < 0 || n_zero < 0) return mdq_set_error("mdq_replay_prio_fill: bad arguments");
  if (n_new > capacity || n_zero > capacity || (n_new > 0 && (base_new < 0 || base_new >= capacity)) ||
      (n_zero > 0 && (base_zero < 0 || base_zero >= capacity)))
    return mdq_set_error("mdq_replay_prio_fill: a range exceeds the capacity");
  if (n_new > 0 && n_zero > 0) {   // circular ranges overlap iff one's first record lies inside the other
    const long long dz = ((long long)base_zero - base_new + capacity) % capacity, dn = ((long long)base_new - base_zero + capacity) % capacity;
    if (dz < n_new || dn < n_zero) return mdq_set_error("mdq_replay_prio_fill: the two ranges overlap");
  }
  const long long m = (long long)n_new + n_zero;
  if (m == 0) return 0;
  hipLaunchKernelGGL(mdq_replay::prio_fill_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, prio,
                     capacity, base_new, n_new, base_zero, n_zero, pmax);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("prio_fill_kernel launch failed");
  return 0;
}

extern "C" int mdq_replay_prio_draw(const mdq_replay_prio_draw_desc* d, void* stream) {
  if (!d || d->capacity <= 0 || d->n < 1 || d->n > mdq_replay::PT || !(d->beta >= 0.0) || !d->prio || !d->u || !d->idx || !d->weight)
    return mdq_set_error("mdq_replay_prio_draw: bad arguments");
  hipLaunchKernelGGL(mdq_replay::prio_draw_kernel, dim3(1), dim3(mdq_replay::PT), 0, (hipStream_t)stream, *d);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("prio_draw_kernel launch failed");
  return 0;
}

extern "C" int mdq_replay_prio_update(float* prio, int32_t capacity, int32_t n, const int32_t* idx, const float* td, double alpha,
                                      double eps, float* pmax, void* stream) {
  if (!prio || !pmax || !idx || !td || capacity <= 0 || n < 1 || n > mdq_replay::PT || !(alpha >= 0.0) || !(eps >= 0.0))
    return mdq_set_error("mdq_replay_prio_update: bad arguments");
  int threads = 64;
  while (threads < n) threads <<= 1;
  hipLaunchKernelGGL(mdq_replay::prio_update_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, prio, capacity, n, idx, td,
                     alpha, eps, pmax);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("prio_update_kernel launch failed");
  return 0;
}

// ---------------------------------------------------------------- stream-concurrency probe
// A kernel that keeps the workgroup dispatcher of its hardware queue busy: `wgs` workgroups that each hold `lds` bytes of
// LDS (one per CU at 150 KB) and spin for `ticks` of the 100 MHz wall clock.  meshdqn_amd/streams.py launches it with
// more workgroups than CUs on one stream and a tiny kernel on another: the tiny kernel finishes at once only if the
// two streams sit on hardware queues that dispatch independently.
namespace mdq_replay {
__global__ __launch_bounds__(64) void spin_kernel(long long ticks, int* sink) {
  extern __shared__ int spin_lds[];
  const long long t0 = wall_clock64();
  int acc = 0;
  while (wall_clock64() - t0 < ticks) acc += 1;
  spin_lds[threadIdx.x] = acc;
  if (sink && acc < 0) sink[0] = spin_lds[0];
}
}  // namespace mdq_replay

extern "C" int mdq_spin(int32_t wgs, int32_t lds_bytes, int64_t ticks_100mhz, void* stream) {
  if (wgs <= 0 || lds_bytes < 256 || lds_bytes > 160 * 1024) return mdq_set_error("mdq_spin: bad arguments");
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mdq_replay::spin_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return mdq_set_error(hipGetErrorString(e));
  hipLaunchKernelGGL(mdq_replay::spin_kernel, dim3(wgs), dim3(64), lds_bytes, (hipStream_t)stream, (long long)ticks_100mhz,
                     (int*)nullptr);
  if (hipGetLastError() != hipSuccess) return mdq_set_error("spin_kernel launch failed");
  return 0;
}

// A stream whose kernels may only be placed on the compute units of `mask` (bit i of word i / 32 = compute unit i in the
// driver's numbering: on a multi-XCD part consecutive bits go round-robin over the XCDs, then over the shader engines of
// an XCD, so "the first half of the bits" is half of every shader engine of every XCD).  meshdqn_amd/streams.py gives the
// main chain and the flow leg of the env step disjoint halves of the chip: both are chains of one-workgroup-per-
// environment kernels (128 workgroups that each want a compute unit of their own), and left to the dispatcher the
// workgroups of the two chains are packed onto shared compute units whenever their LDS fits.
extern "C" int mdq_stream_create_cu_mask(const uint32_t* mask, int32_t nwords, void** stream) {
  if (!mask || nwords <= 0 || !stream) return mdq_set_error("mdq_stream_create_cu_mask: bad arguments");
  hipStream_t s = nullptr;
  hipError_t e = hipExtStreamCreateWithCUMask(&s, (uint32_t)nwords, mask);
  if (e != hipSuccess) return mdq_set_error(hipGetErrorString(e));
  *stream = s;
  return 0;
}

extern "C" int mdq_stream_destroy(void* stream) {
  if (!stream) return 0;
  hipError_t e = hipStreamDestroy((hipStream_t)stream);
  if (e != hipSuccess) return mdq_set_error(hipGetErrorString(e));
  return 0;
}
