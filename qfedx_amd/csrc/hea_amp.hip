// Amplitude-encoded inputs of the MFMA statevector engine: raw features x[s, 0:F] (F <= N = 2^n, zero padded) ->
// psi_in of forward pass 0 in the engine's storage format, one 32-bit word (re, 0) of fp16 or bf16 per amplitude,
// scaled by the engine's power-of-two state scale.  Same semantics as qfx_amp_init (statevec.hip): psi = x / ||x||_2
// with a float64 norm, a row whose norm is not > 0 -> the uniform state 1/sqrt(N).
//
// One launch, one workgroup per sample.  Thread t owns the 16-byte vectors t, t + T, t + 2T, ... of its row (T threads),
// whatever the batch size or the grid: the float64 sum of squares runs per thread in that order, then over the wave
// (xor shuffles), then over the waves in index order, so a row stages to the same bits in any batch.  While the row
// fits the workgroup's registers (N <= 2^15: up to 8 vectors per thread) it is read once and stays in registers
// between the reduction and the write; longer rows are read a second time.  Stores are plain 16-byte vector stores.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int AMP_MAX_THREADS = 1024;
constexpr int AMP_MAX_VECS = 8;                 // register-resident vectors per thread (N <= 2^15)

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };   // a 16-byte load from a 4-byte-aligned row

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// elements [4 vi, 4 vi + 4) of the row, zero from F on; AL: the row starts on a 16-byte boundary
template <bool AL>
__device__ __forceinline__ float4 load_vec(const float* __restrict__ row, long vi, long F) {
  const long i = 4 * vi;
  if (i + 4 <= F) {
    if constexpr (AL) return *reinterpret_cast<const float4*>(row + i);
    const f4u u = *reinterpret_cast<const f4u*>(row + i);
    return make_float4(u.x, u.y, u.z, u.w);
  }
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < F) v.x = row[i];
  if (i + 1 < F) v.y = row[i + 1];
  if (i + 2 < F) v.z = row[i + 2];
  return v;
}

__device__ __forceinline__ double sq_sum(double acc, float4 v) {
  acc += (double)v.x * (double)v.x;
  acc += (double)v.y * (double)v.y;
  acc += (double)v.z * (double)v.z;
  acc += (double)v.w * (double)v.w;
  return acc;
}

template <bool BF16>
__device__ __forceinline__ uint32_t pack_re(float a) {
  if constexpr (BF16) {
    const uint32_t u = __float_as_uint(a);                    // round to nearest even to 8 significand bits
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
  } else {
    const _Float16 h = (_Float16)a;
    return (uint32_t)__builtin_bit_cast(uint16_t, h);
  }
}

template <bool BF16>
__device__ __forceinline__ uint4 encode(float4 v, bool zero, double inv, float uni, float scale) {
  const float a0 = zero ? uni : (float)((double)v.x * inv), a1 = zero ? uni : (float)((double)v.y * inv);
  const float a2 = zero ? uni : (float)((double)v.z * inv), a3 = zero ? uni : (float)((double)v.w * inv);
  return make_uint4(pack_re<BF16>(a0 * scale), pack_re<BF16>(a1 * scale), pack_re<BF16>(a2 * scale),
                    pack_re<BF16>(a3 * scale));
}

template <int V, bool BF16, bool AL>
__device__ __forceinline__ void stage_row(const float* __restrict__ row, long F, long N, uint32_t* __restrict__ dst,
                                          float scale, double* sm) {
  const int T = blockDim.x, tid = threadIdx.x;
  const long nvec = N >> 2;
  float4 v[V > 0 ? V : 1];
  double acc = 0.0;
  if constexpr (V > 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = load_vec<AL>(row, (long)j * T + tid, F);
#pragma unroll
    for (int j = 0; j < V; ++j) acc = sq_sum(acc, v[j]);
  } else {
    for (long vi = tid; vi < nvec; vi += T) acc = sq_sum(acc, load_vec<AL>(row, vi, F));
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) sm[tid >> 6] = acc;
  __syncthreads();
  double nrm2 = 0.0;
  for (int w = 0; w < (T + 63) / 64; ++w) nrm2 += sm[w];
  const bool zero = !(nrm2 > 0.0);
  const double inv = zero ? 0.0 : 1.0 / sqrt(nrm2);
  const float uni = (float)(1.0 / sqrt((double)N));
  uint4* out = reinterpret_cast<uint4*>(dst);
  if constexpr (V > 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) out[(long)j * T + tid] = encode<BF16>(v[j], zero, inv, uni, scale);
  } else {
    for (long vi = tid; vi < nvec; vi += T)
      out[vi] = encode<BF16>(load_vec<AL>(row, vi, F), zero, inv, uni, scale);
  }
}

// V > 0: V vectors per thread, kept in registers (N = 4 V blockDim.x); V = 0: any N, the row is read twice.  A row
// that starts off a 16-byte boundary (a row stride that is no multiple of 4 elements) is read with 4-byte loads into
// the same registers: the values, the summation order and the stores are those of an aligned row.
template <int V, bool BF16>
__global__ void __launch_bounds__(AMP_MAX_THREADS) hea_amp_stage_kernel(const float* __restrict__ x, long F, long ld,
                                                                        long N, uint32_t* __restrict__ psi,
                                                                        float scale) {
  __shared__ double sm[AMP_MAX_THREADS / 64];
  const long s = blockIdx.x;
  const float* row = x + s * ld;
  if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) stage_row<V, BF16, true>(row, F, N, psi + s * N, scale, sm);
  else stage_row<V, BF16, false>(row, F, N, psi + s * N, scale, sm);
}

template <bool BF16>
void launch(const float* x, long F, long ld, int S, long N, uint32_t* psi, float scale, hipStream_t st) {
  const long nvec = N >> 2;
  const int T = (int)(nvec < 64 ? 64 : nvec > AMP_MAX_THREADS ? AMP_MAX_THREADS : nvec);
  const long per = nvec / T;
  const dim3 grid((unsigned)S), block((unsigned)T);
#define QFX_AMP(VV) hipLaunchKernelGGL((hea_amp_stage_kernel<VV, BF16>), grid, block, 0, st, x, F, ld, N, psi, scale)
  if (per == 1 && nvec == T) QFX_AMP(1);
  else if (per == 2) QFX_AMP(2);
  else if (per == 4) QFX_AMP(4);
  else if (per == AMP_MAX_VECS) QFX_AMP(8);
  else QFX_AMP(0);
#undef QFX_AMP
}

}  // namespace

// x [S, F] fp32 with row stride ld (elements), psi [S * 2^n] words, 16-byte aligned.  n >= 8 (a row is at least 64
// vectors: every thread of the smallest workgroup owns one).
extern "C" int qfx_hea_amp_stage(const float* x, long F, long ld, int S, int n, uint32_t* psi, float scale, int bf16,
                                 hipStream_t st) {
  if (n < 8 || n > 30 || F <= 0 || F > (1L << n) || ld < F || S <= 0) return -2;
  if (reinterpret_cast<uintptr_t>(psi) & 15) return -3;
  const long N = 1L << n;
  if (bf16) launch<true>(x, F, ld, S, N, psi, scale, st);
  else launch<false>(x, F, ld, S, N, psi, scale, st);
  return (int)hipGetLastError();
}
