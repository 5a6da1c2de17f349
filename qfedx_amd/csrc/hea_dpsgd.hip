// Record-level DP-SGD on the MFMA statevector engine: per-sample clipping and the noised lot sum, from what a training
// step already wrote - the adjoint passes' per-sample gradient slab gslab[sample][tile][gradop][32] (int64 fixed
// point) and the per-sample readout records rorec[sample][2C + 2] (hea_step.hip hea_readout_rec_kernel) - so no
// circuit is evaluated again.  Two launches take the place of hea_grad_reduce:
//
//   hea_dp_norm    per sample s: the l2 norm of its whole gradient row (n_theta circuit entries through the shared
//                  per-gradop formulas of hea_gradop.h, 2C readout entries) and c_s = min(1, C / max(norm, 1e-12))
//   hea_dp_reduce  per client k: grad[k][i] = (sum_s c_s g_s[i] + sigma C z_{k,i}) / lot, formed from the weighted slab
//                  sums (a per-sample gradient is linear in its slab row at fixed theta), z from the client's Philox key
//                  read from a device table, and the client's loss (mean CE over the lot's live samples) and hits
//
// Storage independent (the slab and the records are the same for fp16 and bf16 states): compiled once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hea_gradop.h"
#include "philox.h"

namespace qfx_dp {

constexpr double FIX = 4294967296.0;   // 2^32: fixed point of the slab (hea_common.h)

// One block per sample.  8 groups of 32 lanes take the gradient ops 8 at a time; lane l of a group sums slot l over the
// op's tiles (exact int64 sums, 8 tile loads in flight), lanes < nreal turn the sums into (d/dtheta, d/dphi) and square
// them.  Squares are accumulated in double and combined in a fixed order.
__global__ void __launch_bounds__(256) hea_dp_norm_kernel(const long long* __restrict__ gslab, int slab_tiles,
                                                          int n_gradops, const int* __restrict__ gmeta, int spc,
                                                          const float* __restrict__ params, int p_stride,
                                                          const float* __restrict__ rec, int C, double clip,
                                                          double* __restrict__ norm, double* __restrict__ cfac) {
  const long s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 31, grp = tid >> 5;
  const float* prm = params + (size_t)(s / spc) * p_stride;
  __shared__ double pt[8][32];
  __shared__ double red[256];
  double acc = 0.0;
  for (int g0 = 0; g0 < n_gradops; g0 += 8) {
    const int g = g0 + grp;
    const bool on = g < n_gradops;
    const int* m = gmeta + (on ? g : 0) * 10;
    const int nt = on ? m[0] : 0, nreal = m[1] & 15, inside = (m[1] >> 4) & 1;
    auto row = [&](int t) -> long long {
      return gslab[(((size_t)s * slab_tiles + t) * n_gradops + g) * 32 + lane];
    };
    constexpr int TU = 8;
    long long tot = 0;
    int t = 0;
    for (; t + TU <= nt; t += TU) {
      long long v[TU];
#pragma unroll
      for (int u = 0; u < TU; ++u) v[u] = row(t + u);
#pragma unroll
      for (int u = 0; u < TU; ++u) tot += v[u];
    }
    for (; t < nt; ++t) tot += row(t);
    pt[grp][lane] = (double)tot / FIX;
    __syncthreads();
    if (on && lane < nreal) {
      double gth, gph;
      qfx::hea_gradop_pair(pt[grp], prm, m, lane, inside, gth, gph);
      acc += gth * gth + gph * gph;
    }
    __syncthreads();
  }
  if (tid < 2 * C) {       // the readout gradients of the sample: d/da_c = dl_c z_c, d/db_c = dl_c
    const double v = rec[(size_t)s * (2 * C + 2) + tid];
    acc += v * v;
  }
  red[tid] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double nn = sqrt(red[0]);
    norm[s] = nn;
    cfac[s] = fmin(1.0, clip / fmax(nn, 1e-12));       // the rule of privacy/dp.py clip_factors
  }
}

// Grid (client, gradient op + 1 readout block), as hea_grad_reduce.  The weighted sums run in double in an order that
// depends only on (spc, nt): group grp takes rows grp, grp + 8, ... of the client's (sample, tile) rows in turn, and the
// 8 group partials are added in group order.
__global__ void __launch_bounds__(256) hea_dp_reduce_kernel(const long long* __restrict__ gslab, int slab_tiles,
                                                            int n_gradops, const int* __restrict__ gmeta, int spc,
                                                            const float* __restrict__ params, int p_stride,
                                                            const float* __restrict__ rec, const float* __restrict__ wts,
                                                            const double* __restrict__ cfac, int C, int n_theta,
                                                            const long long* __restrict__ keys, long long step,
                                                            double sigma, double clip, double lot,
                                                            float* __restrict__ grad, float* __restrict__ loss,
                                                            float* __restrict__ correct) {
  const int k = blockIdx.x, g = blockIdx.y, tid = threadIdx.x, lane = tid & 31, grp = tid >> 5;
  const int P = n_theta + 2 * C;
  // entry i of the client's row: the weighted sum plus the client's noise element step P + i, over the nominal lot size
  auto finish = [&](int i, double sum) {
    double v = sum;
    if (sigma > 0.0) {
      const unsigned long long k0 = (unsigned long long)keys[2 * k], k1 = (unsigned long long)keys[2 * k + 1];
      const double z = qfx::philox_normal_at((uint64_t)step * (uint64_t)P + (uint64_t)i, (uint32_t)k0, (uint32_t)k1, 0u);
      v += sigma * clip * z;
    }
    grad[(size_t)k * p_stride + i] = (float)(v / lot);
  };
  if (g == n_gradops) {
    // readout block: per sample the 2C clipped readout gradients, the loss term, the hit and the live flag.  Thread
    // t < GS * NV sums value q = t % NV of samples t / NV + GS i (contiguous loads, all in flight), then thread q sums
    // the GS partials in order (the layout of hea_grad_reduce's readout block).
    __shared__ double rs[256];
    __shared__ double tots[19];
    const int NR = 2 * C + 2, NV = NR + 1, GS = 256 / NV;
    const float* rk = rec + (size_t)k * spc * NR;
    double v = 0.0;
    if (tid < GS * NV) {
      const int q = tid % NV;
      for (int j = tid / NV; j < spc; j += GS) {
        if (q < 2 * C)
          v += cfac[(size_t)k * spc + j] * (double)rk[j * NR + q];
        else if (q < NR)
          v += (double)rk[j * NR + q];
        else
          v += wts[(size_t)k * spc + j] > 0.f ? 1.0 : 0.0;
      }
    }
    rs[tid] = v;
    __syncthreads();
    if (tid < NV) {
      double tot = 0.0;
      for (int j = 0; j < GS; ++j) tot += rs[j * NV + tid];
      tots[tid] = tot;
      if (tid < 2 * C) finish(n_theta + tid, tot);
    }
    __syncthreads();
    if (tid == 0) {
      const double live = tots[NR];
      loss[k] = live > 0.0 ? (float)(tots[2 * C] / live) : 0.f;     // mean CE over the lot's live samples
      correct[k] = (float)tots[2 * C + 1];
    }
    return;
  }
  const int* m = gmeta + g * 10;
  const int nt = m[0], nreal = m[1] & 15, inside = (m[1] >> 4) & 1;
  const int R = spc * nt;
  __shared__ double part[8][32];
  __shared__ double pt[32];
  auto row = [&](int r) -> long long {
    const int s = k * spc + r / nt, t = r % nt;
    return gslab[(((size_t)s * slab_tiles + t) * n_gradops + g) * 32 + lane];
  };
  auto cf = [&](int r) -> double { return cfac[(size_t)k * spc + r / nt]; };
  // RU rows per lane in flight, as in hea_grad_reduce (the slab rows come from other XCDs' passes, an L2 miss each)
  constexpr int RU = 16;
  double tot = 0.0;
  int r = grp;
  for (; r + 8 * (RU - 1) < R; r += 8 * RU) {
    long long v[RU];
    double c[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) v[u] = row(r + 8 * u), c[u] = cf(r + 8 * u);
#pragma unroll
    for (int u = 0; u < RU; ++u) tot += c[u] * (double)v[u];
  }
  for (; r < R; r += 8) tot += cf(r) * (double)row(r);
  part[grp][lane] = tot;
  __syncthreads();
  if (tid < 32) {
    double v = 0.0;
    for (int j = 0; j < 8; ++j) v += part[j][tid];
    pt[tid] = v / FIX;
  }
  __syncthreads();
  if (tid < nreal) {
    double gth, gph;
    qfx::hea_gradop_pair(pt, params + (size_t)k * p_stride, m, tid, inside, gth, gph);
    finish(m[2 + tid], gth);
    finish(m[6 + tid], gph);
  }
}

}  // namespace qfx_dp

extern "C" int qfx_hea_dp_norm(const long long* gslab, int slab_tiles, int n_gradops, const int* gmeta, int spc, int K,
                               const float* params, int p_stride, const float* rec, int C, int n_theta, double clip,
                               double* norm, double* cfac, hipStream_t st) {
  const long S = (long)K * spc;
  if (S == 0) return 0;
  if (C < 1 || C > 8 || spc < 1 || n_theta + 2 * C > p_stride || S > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(qfx_dp::hea_dp_norm_kernel, dim3((unsigned)S), dim3(256), 0, st, gslab, slab_tiles, n_gradops,
                     gmeta, spc, params, p_stride, rec, C, clip, norm, cfac);
  return (int)hipGetLastError();
}

extern "C" int qfx_hea_dp_reduce(const long long* gslab, int slab_tiles, int n_gradops, const int* gmeta, int spc, int K,
                                 const float* params, int p_stride, const float* rec, const float* wts,
                                 const double* cfac, int C, int n_theta, const long long* keys, long long step,
                                 double sigma, double clip, double lot, float* grad, float* loss, float* correct,
                                 hipStream_t st) {
  if (K == 0) return 0;
  if (C < 1 || C > 8 || spc < 1 || n_theta + 2 * C > p_stride || !(lot > 0.0) || sigma < 0.0 || step < 0 ||
      (sigma > 0.0 && !keys))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(qfx_dp::hea_dp_reduce_kernel, dim3(K, n_gradops + 1), dim3(256), 0, st, gslab, slab_tiles,
                     n_gradops, gmeta, spc, params, p_stride, rec, wts, cfac, C, n_theta, keys, step, sigma, clip, lot,
                     grad, loss, correct);
  return (int)hipGetLastError();
}
