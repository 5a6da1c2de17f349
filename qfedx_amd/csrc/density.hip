// Exact density-matrix simulation of small noisy circuits (ROADMAP.md:64-73: depolarizing p, amplitude damping
// gamma as their exact Kraus channels; the statevector engines only realise Pauli channels, as trajectories).
//
// rho (2^n x 2^n, complex64) is a vector over 2n index bits: bit q of a row index is bit q, bit q of a column
// index is bit q + n (i = r + c 2^n).  A one-qubit gate U on qubit q followed by the gate-noise channel {K_i}
// on q is ONE 4 x 4 superoperator on the bit pair (q, q + n):
//     T = S (U (x) U*),   S[(a, b)][(a', b')] = sum_i K_i[a][a'] conj(K_i[b][b'])   (quad element a + 2 b)
// applied to every quad of rho in one pass.  Two-qubit gates (cx, cz, swap) are permutations / signs of rows and
// columns (in-place pair swaps), followed by S on each qubit they touch.  <Z_c> = sum_r rho_rr (1 - 2 r_c).
// The channel is trace preserving, so nothing renormalises.
//
// One workgroup runs one circuit instance (one sample row of slot values) through the whole program: rho lives
// in LDS up to n = 6 (32 KB) and in a global scratch slab beyond (n <= 10; 512 KB at n = 8 stays in the XCD's
// L2).  Passes are separated by workgroup barriers (the L1 is shared by a workgroup's waves, so a workgroup-scope
// fence orders the global slab too).  ops/density.py lowers the program; quantum/noise.py is the float64 oracle.
#include "dm_common.h"

namespace dm {

struct Args {
  const Gate* gates;
  int G, n;
  const float* rows;   // [S][W] slot values (theta | x)
  int W;
  const int* readout;
  int C;
  const float* S;      // [32] noise superoperator (re, im) x 16, row-major over quad index a + 2 b; null = none
  float2* scratch;     // [S][4^n] when n > LDS_QUBITS
  float* expz;         // [S][C]
};

__global__ void __launch_bounds__(NT) dm_kernel(Args a) {
  __shared__ float2 rho_s[1 << (2 * LDS_QUBITS)];
  __shared__ float2 T[16];
  __shared__ float red[NT / 64][CMAX];
  const int s = blockIdx.x, n = a.n;
  const long N = 1L << (2 * n);
  float2* rho = n <= LDS_QUBITS ? rho_s : a.scratch + (size_t)s * N;
  const float* row = a.rows + (size_t)s * a.W;
  for (long i = threadIdx.x; i < N; i += NT) rho[i] = make_float2(i == 0 ? 1.f : 0.f, 0.f);
  __syncthreads();
  for (int gi = 0; gi < a.G; ++gi) {
    const Gate g = a.gates[gi];
    if (g.kind == K_CX || g.kind == K_CZ || g.kind == K_SWAP) {
      if (g.kind == K_CZ) {
        apply_cz(rho, n, g.q0, g.q1);
      } else {
        permute_side(rho, n, g.kind, g.q0, g.q1, 0);
        __syncthreads();
        permute_side(rho, n, g.kind, g.q0, g.q1, n);
      }
      if (a.S) {                               // the channel on both qubits
        const float2 id[4] = {make_float2(1.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(1.f, 0.f)};
        __syncthreads();
        build_superop(id, a.S, T);
        __syncthreads();
        apply_superop(rho, n, g.q0, T);
        __syncthreads();
        apply_superop(rho, n, g.q1, T);
      }
    } else {
      float2 u[4];
      gate_matrix(g, row, u);
      build_superop(u, a.S, T);
      __syncthreads();
      apply_superop(rho, n, g.q0, T);
    }
    __syncthreads();
  }
  // <Z_c> from the diagonal, fixed-order block reduction
  const long D = 1L << n;
  float acc[CMAX];
  for (int c = 0; c < a.C; ++c) acc[c] = 0.f;
  for (long r = threadIdx.x; r < D; r += NT) {
    const float p = rho[r + (r << n)].x;
    for (int c = 0; c < a.C; ++c) acc[c] += ((r >> a.readout[c]) & 1) ? -p : p;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = 0; c < a.C; ++c) {
    float v = acc[c];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < a.C) {
    float v = 0.f;
    for (int w = 0; w < NT / 64; ++w) v += red[w][threadIdx.x];
    a.expz[(size_t)s * a.C + threadIdx.x] = v;
  }
}

}  // namespace dm

extern "C" int qfx_dm_gate_bytes() { return (int)sizeof(dm::Gate); }

extern "C" int qfx_dm_run(const void* gates, int G, int n, const float* rows, int W, long S, const int* readout, int C,
                          const float* superop, void* scratch, float* expz, hipStream_t st) {
  if (n < 1 || n > dm::MAXQ || C < 1 || C > dm::CMAX || S <= 0) return (int)hipErrorInvalidValue;
  if (n > dm::LDS_QUBITS && !scratch) return (int)hipErrorInvalidValue;
  dm::Args a{(const dm::Gate*)gates, G, n, rows, W, readout, C, superop, (float2*)scratch, expz};
  hipLaunchKernelGGL(dm::dm_kernel, dim3((unsigned)S), dim3(dm::NT), 0, st, a);
  return (int)hipGetLastError();
}

extern "C" int qfx_dm_lds_qubits() { return dm::LDS_QUBITS; }
