// Quantum natural gradient: the Fubini-Study metric blocks of the hardware-efficient ansatz and the damped natural
// step (ops/qng.py; Stokes et al. 2020, block-diagonal approximation).
//
// A sublayer's block is g_ij = 1/4 (<Z_i Z_j> - <Z_i><Z_j>) on its reference state (RX sublayers: on H^n psi, where
// the X correlators are Z correlators), so the metric needs <Z_i> and <Z_i Z_j> of p(x) = |psi_x|^2 for every sample:
//
//   qng_corr_tile   per (sample, tile of 2^11 amplitudes): the Walsh-Hadamard transform W of the tile's probabilities,
//                   W[m] = sum_x (-1)^{|m & x|} p(x), read at the weight <= 2 indices: W[0] is the tile's probability,
//                   W[1 << i] its low-bit single sums, W[(1 << i) | (1 << j)] its low-low pair sums.  One sweep of
//                   the state, 11 butterfly stages per amplitude instead of n^2 / 2 signed sums.
//   qng_corr_comb   per sample: the tile records summed over tiles in tile order (float64).  For a pair with a high
//                   bit the sign is constant per tile: low x high = sum_t s_j(t) W_t[1 << i], high x high =
//                   sum_t s_i(t) s_j(t) W_t[0].  Writes the sample's record rec[sample][cut][n (n + 1) / 2] =
//                   [<Z_0> .. <Z_{n-1}> | <Z_i Z_j>, i < j, row-major].
//   qng_step        per (client, block): G = mean over the client's live samples (wmask > 0, in sample order) of
//                   1/4 (<Z_i Z_j> - <Z_i><Z_j>), diagonal 1/4 (1 - <Z_i>^2); G + lambda I = L L^T in LDS (float64);
//                   theta_block -= lr (G + lambda I)^{-1} grad_block on active rows.  The last block column of the
//                   grid takes the plain step on the readout entries a / b.  qng_blocks writes G itself (no lambda).
//
// Every sum has a fixed order and no atomics: a sample's record does not depend on the samples it shares a launch
// with, and a client's step does not depend on its batch mates.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qfx_qng {

constexpr int TB = 11;                       // tile bits: 256 lanes x 4 x (2 amplitudes per 16-byte load)
constexpr int TILE = 1 << TB;
constexpr int TREC = 1 + TB + TB * (TB - 1) / 2;   // tile record: W[0], singles, pairs (i < j, row-major)
constexpr int NMAX = 32;

__device__ __forceinline__ int pair_index(int i, int j, int n) {   // i < j < n, row-major over the upper triangle
  return i * n - i * (i + 1) / 2 + (j - i - 1);
}

// Tile element e = 2 f + c with f = tid + 256 j the tile's 16-byte load index: index bit 0 = c and bits 9, 10 = j live
// in a lane's registers, bits 1..6 are the lane id (cross-lane butterflies), bits 7, 8 the wave id (two LDS stages).
// A state shorter than the tile (n < 11) is padded with zero probabilities: W at indices below 2^n is unchanged.
__global__ void __launch_bounds__(256) qng_corr_tile_kernel(const float4* __restrict__ states, int n, long tiles,
                                                            float* __restrict__ trec) {
  __shared__ float w[TILE];
  const long blk = blockIdx.x;               // sample * tiles + tile
  const int tid = threadIdx.x, lane = tid & 63;
  const int tbits = n < TB ? n : TB;
  const int nload = 1 << (tbits - 1);        // 16-byte loads that hold the tile
  const float4* src = states + blk * (long)nload;   // tiles > 1 only when nload = TILE / 2: consecutive tiles
  float v[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int f = tid + 256 * j;
    float p0 = 0.f, p1 = 0.f;
    if (f < nload) {
      const float4 a = src[f];
      p0 = a.x * a.x + a.y * a.y;
      p1 = a.z * a.z + a.w * a.w;
    }
    v[j][0] = p0 + p1;                       // bit 0
    v[j][1] = p0 - p1;
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {              // bits 9, 10
    const float a0 = v[0][c] + v[1][c], a1 = v[0][c] - v[1][c], a2 = v[2][c] + v[3][c], a3 = v[2][c] - v[3][c];
    v[0][c] = a0 + a2;
    v[1][c] = a1 + a3;
    v[2][c] = a0 - a2;
    v[3][c] = a1 - a3;
  }
#pragma unroll
  for (int b = 0; b < 6; ++b) {              // bits 1..6 = lane bits 0..5
    const bool hi = (lane >> b) & 1;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float o = __shfl_xor(v[j][c], 1 << b, 64);
        v[j][c] = hi ? o - v[j][c] : v[j][c] + o;
      }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<float2*>(&w[2 * (tid + 256 * j)]) = make_float2(v[j][0], v[j][1]);
  __syncthreads();
#pragma unroll
  for (int b = 7; b < 9; ++b) {              // bits 7, 8 = wave id: strides of 128 / 256 floats, conflict free
    const int h = 1 << b;
    float lo[4], up[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = tid + 256 * r;           // butterfly index, 1024 per stage
      const int i = ((q >> b) << (b + 1)) | (q & (h - 1));
      lo[r] = w[i];
      up[r] = w[i + h];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = tid + 256 * r;
      const int i = ((q >> b) << (b + 1)) | (q & (h - 1));
      w[i] = lo[r] + up[r];
      w[i + h] = lo[r] - up[r];
    }
    __syncthreads();
  }
  float* out = trec + blk * TREC;
  if (tid == 0) out[0] = w[0];
  if (tid >= 64 && tid < 64 + TB) out[1 + (tid - 64)] = w[1 << (tid - 64)];
  if (tid >= 128 && tid < 128 + TB * (TB - 1) / 2) {
    int i = 0, r = tid - 128;
    while (r >= TB - 1 - i) r -= TB - 1 - i, ++i;
    const int j = i + 1 + r;
    out[1 + TB + (tid - 128)] = w[(1 << i) | (1 << j)];
  }
}

// One block per sample; thread o sums output o (n singles, then the pairs) over the sample's tiles in tile order.
__global__ void __launch_bounds__(256) qng_corr_comb_kernel(const float* __restrict__ trec, int n, long tiles,
                                                            double* __restrict__ rec, long rec_stride) {
  const long s = blockIdx.x;
  const int tbits = n < TB ? n : TB;
  const int nout = n + n * (n - 1) / 2;
  const float* base = trec + s * tiles * TREC;
  double* out = rec + s * rec_stride;
  for (int o = threadIdx.x; o < nout; o += blockDim.x) {
    int i, j = -1;
    if (o < n) {
      i = o;
    } else {
      int r = o - n;
      i = 0;
      while (r >= n - 1 - i) r -= n - 1 - i, ++i;
      j = i + 1 + r;
    }
    // the tile-record entry that carries the low part, and the high bits whose sign multiplies it
    int ent, h0 = -1, h1 = -1;
    if (j < 0) {
      if (i < tbits) ent = 1 + i; else ent = 0, h0 = i - tbits;
    } else if (j < tbits) {
      ent = 1 + TB + pair_index(i, j, TB);
    } else if (i < tbits) {
      ent = 1 + i, h0 = j - tbits;
    } else {
      ent = 0, h0 = i - tbits, h1 = j - tbits;
    }
    double acc = 0.0;
    for (long t = 0; t < tiles; ++t) {
      const double x = (double)base[t * TREC + ent];
      int neg = 0;
      if (h0 >= 0) neg ^= (int)((t >> h0) & 1);
      if (h1 >= 0) neg ^= (int)((t >> h1) & 1);
      acc += neg ? -x : x;
    }
    out[o] = acc;
  }
}

// G[i][j] (i, j < n; g row stride NMAX) of (client k, block b) from the per-sample records; returns the live count.
__device__ int form_block(const double* __restrict__ rec, const float* __restrict__ wmask, int k, int b, int B,
                          int nblk, int n, double* g) {
  const int R = n * (n + 1) / 2;
  int live = 0;
  for (int s = 0; s < B; ++s) live += wmask[(long)k * B + s] > 0.f ? 1 : 0;
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
    const int i = e / n, j = e % n;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double acc = 0.0;
    for (int s = 0; s < B; ++s) {
      if (!(wmask[(long)k * B + s] > 0.f)) continue;
      const double* r = rec + (((long)k * B + s) * nblk + b) * R;
      const double zi = r[lo], zj = r[hi];
      const double zz = lo == hi ? 1.0 : r[n + pair_index(lo, hi, n)];
      acc += 0.25 * (zz - zi * zj);
    }
    g[i * NMAX + j] = live > 0 ? acc / (double)live : 0.0;
  }
  return live;
}

__global__ void __launch_bounds__(256) qng_blocks_kernel(const double* __restrict__ rec,
                                                         const float* __restrict__ wmask, int B, int nblk, int n,
                                                         double* __restrict__ out) {
  __shared__ double g[NMAX * NMAX];
  const int k = blockIdx.x, b = blockIdx.y;
  form_block(rec, wmask, k, b, B, nblk, n, g);
  __syncthreads();
  double* o = out + ((long)k * nblk + b) * n * n;
  for (int e = threadIdx.x; e < n * n; e += blockDim.x) o[e] = g[(e / n) * NMAX + (e % n)];
}

// grid (K, nblk + 1): block column b < nblk solves sublayer b, column nblk steps the params past n_theta.
__global__ void __launch_bounds__(256) qng_step_kernel(const double* __restrict__ rec, const float* __restrict__ wmask,
                                                       int B, int nblk, int n, const float* __restrict__ grad,
                                                       const float* __restrict__ active, float* __restrict__ params,
                                                       int P, double lr, double damping) {
  __shared__ double g[NMAX * NMAX];
  __shared__ double rhs[NMAX];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (!(active[k] > 0.f)) return;            // (uniform per block) inactive rows keep their bits
  float* p = params + (long)k * P;
  const float* gr = grad + (long)k * P;
  const int n_theta = n * nblk;
  if (b == nblk) {
    for (int i = n_theta + tid; i < P; i += blockDim.x) p[i] = (float)((double)p[i] - lr * (double)gr[i]);
    return;
  }
  form_block(rec, wmask, k, b, B, nblk, n, g);
  // entry i of block b = 2 l + r is the flat angle 2 (n l + i) + r
  const int base = 2 * n * (b >> 1) + (b & 1);
  if (tid < n) rhs[tid] = (double)gr[base + 2 * tid];
  __syncthreads();
  if (tid < n) g[tid * NMAX + tid] += damping;
  __syncthreads();
  // right-looking Cholesky on the lower triangle, L in place
  for (int c = 0; c < n; ++c) {
    if (tid == 0) g[c * NMAX + c] = sqrt(g[c * NMAX + c]);
    __syncthreads();
    if (tid > c && tid < n) g[tid * NMAX + c] /= g[c * NMAX + c];
    __syncthreads();
    for (int e = tid; e < n * n; e += blockDim.x) {
      const int i = e / n, j = e % n;
      if (j > c && i >= j) g[i * NMAX + j] -= g[i * NMAX + c] * g[j * NMAX + c];
    }
    __syncthreads();
  }
  for (int c = 0; c < n; ++c) {              // L y = rhs
    if (tid == 0) rhs[c] /= g[c * NMAX + c];
    __syncthreads();
    if (tid > c && tid < n) rhs[tid] -= g[tid * NMAX + c] * rhs[c];
    __syncthreads();
  }
  for (int c = n - 1; c >= 0; --c) {         // L^T x = y
    if (tid == 0) rhs[c] /= g[c * NMAX + c];
    __syncthreads();
    if (tid < c) rhs[tid] -= g[c * NMAX + tid] * rhs[c];
    __syncthreads();
  }
  if (tid < n) p[base + 2 * tid] = (float)((double)p[base + 2 * tid] - lr * rhs[tid]);
}

}  // namespace qfx_qng

extern "C" {

int qfx_qng_tile_rec() { return qfx_qng::TREC; }

long qfx_qng_tiles(int n) { return n > qfx_qng::TB ? 1L << (n - qfx_qng::TB) : 1L; }

// states [S, 2^n] complex64 (16-byte aligned) -> rec[s * rec_stride + 0 .. n (n + 1) / 2); trec: S * tiles * TREC floats
int qfx_launch_qng_corr(const void* states, long S, int n, float* trec, double* rec, long rec_stride,
                        hipStream_t st) {
  using namespace qfx_qng;
  if (n < 1 || n > NMAX || S <= 0) return S == 0 ? 0 : -1;
  const long tiles = qfx_qng_tiles(n);
  if (S * tiles > 0x7fffffffL) return -2;
  hipLaunchKernelGGL(qng_corr_tile_kernel, dim3((unsigned)(S * tiles)), dim3(256), 0, st,
                     static_cast<const float4*>(states), n, tiles, trec);
  hipLaunchKernelGGL(qng_corr_comb_kernel, dim3((unsigned)S), dim3(256), 0, st, trec, n, tiles, rec, rec_stride);
  return (int)hipGetLastError();
}

int qfx_launch_qng_blocks(const double* rec, const float* wmask, int K, int B, int nblk, int n, double* out,
                          hipStream_t st) {
  using namespace qfx_qng;
  if (n < 1 || n > NMAX || K <= 0 || nblk <= 0) return (K == 0 || nblk == 0) ? 0 : -1;
  hipLaunchKernelGGL(qng_blocks_kernel, dim3((unsigned)K, (unsigned)nblk), dim3(256), 0, st, rec, wmask, B, nblk, n,
                     out);
  return (int)hipGetLastError();
}

int qfx_launch_qng_step(const double* rec, const float* wmask, int K, int B, int nblk, int n, const float* grad,
                        const float* active, float* params, int P, double lr, double damping, hipStream_t st) {
  using namespace qfx_qng;
  if (n < 1 || n > NMAX || K <= 0) return K == 0 ? 0 : -1;
  if (P < n * nblk) return -2;
  hipLaunchKernelGGL(qng_step_kernel, dim3((unsigned)K, (unsigned)(nblk + 1)), dim3(256), 0, st, rec, wmask, B, nblk,
                     n, grad, active, params, P, lr, damping);
  return (int)hipGetLastError();
}

}  // extern "C"
