// Reverse-mode gradients of the density-matrix simulator (density.hip): d<O>/d(angle) of every parametrised
// one-qubit gate for <O> = sum_c w_c <Z_c>, from one forward and one backward sweep per sample row.
//
// With <A, B> = sum_i conj(A_i) B_i over the 4^n entries, <O> = <Lambda_G, rho_G> where Lambda_G is diagonal and
// real: Lambda[r, r] = sum_c w_c (1 - 2 r_c).  Every gate is a linear map on rho (the 4 x 4 superoperator
// T = S (U (x) U*) on the quads of its qubit; a permutation / sign followed by S on both qubits for cx, cz, swap),
// so Lambda pulls back through gate g as Lambda_{g-1} = T_g^dagger Lambda_g.  A rotation U = exp(-i ang P / 2) has
// dT/d(ang) = T Gen with Gen rho = -(i / 2) [P, rho] on the same quads (Gen commutes with U (x) U*), hence
//     d<O>/d(ang_g) = Re <T_g^dagger Lambda_g, Gen rho_{g-1}>.
// p(phi) differs from rz(phi) by a global phase, which drops out of U rho U^dagger: it takes rz's Gen.
//
// The channels cannot be run backwards (amplitude damping's inverse grows like (1 - gamma)^-G), so the forward
// sweep stores rho_{g-1} for every differentiated gate - the tape [S][J][4^n], J = the number of parametrised
// one-qubit gates whose slot lies in [0, n_grad), in program order:
//   * dm_tape_kernel   dm_kernel's gate loop, copying rho to the tape in front of each such gate; <Z_c> as dm_kernel
//   * dm_adjoint_kernel  seeds Lambda, walks the gates last to first; at taped gate j ONE pass over the quads forms
//                        Lambda' = T^dagger Lambda in place and the thread's share of Re <Lambda', Gen rho_{g-1}>,
//                        reduced in a fixed order (xor butterfly in the wave, then the waves in order through LDS)
// One workgroup per sample row in both; rho / Lambda in LDS up to n = 6 and in a global slab beyond.  No atomics:
// a row's result does not depend on the other rows of the launch.  Superoperators come from gate_matrix and
// build_superop (dm_common.h) in both directions, which is what makes T^dagger the exact adjoint of the forward map.
#include "dm_common.h"

namespace dm {

struct TapeArgs {
  const Gate* gates;
  int G, n;
  const float* rows;   // [S][W] slot values (theta | x)
  int W;
  const int* readout;
  int C;
  const float* S;      // [32] noise superoperator, null = none (density.hip)
  float2* scratch;     // [S][4^n] when n > LDS_QUBITS
  int n_grad, J;
  float2* tape;        // [S][J][4^n]
  float* expz;         // [S][C]
};

struct AdjArgs {
  const Gate* gates;
  int G, n;
  const float* rows;
  int W;
  const int* readout;
  int C;
  const float* S;
  int n_grad, J;
  const float2* tape;  // [S][J][4^n]
  float2* lam;         // [S][4^n] when n > LDS_QUBITS
  const float* w;      // [S][C] d<O>/d<Z_c>
  float* gg;           // [S][G] d<O>/d(angle of gate g); 0 for gates that are not differentiated
};

__device__ __forceinline__ bool taped(const Gate& g, int n_grad) {
  return g.kind <= K_P && g.slot >= 0 && g.slot < n_grad;
}

__global__ void __launch_bounds__(NT) dm_tape_kernel(TapeArgs a) {
  __shared__ float2 rho_s[1 << (2 * LDS_QUBITS)];
  __shared__ float2 T[16];
  __shared__ float red[NT / 64][CMAX];
  const int s = blockIdx.x, n = a.n;
  const long N = 1L << (2 * n);
  float2* rho = n <= LDS_QUBITS ? rho_s : a.scratch + (size_t)s * N;
  const float* row = a.rows + (size_t)s * a.W;
  for (long i = threadIdx.x; i < N; i += NT) rho[i] = make_float2(i == 0 ? 1.f : 0.f, 0.f);
  __syncthreads();
  int j = 0;
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
      if (taped(g, a.n_grad)) {                // rho_{g-1}; the barrier behind build_superop orders it before the pass
        if (j < a.J) {
          float2* t = a.tape + ((size_t)s * a.J + j) * N;
          for (long i = threadIdx.x; i < N; i += NT) t[i] = rho[i];
        }
        ++j;
      }
      float2 u[4];
      gate_matrix(g, row, u);
      build_superop(u, a.S, T);
      __syncthreads();
      apply_superop(rho, n, g.q0, T);
    }
    __syncthreads();
  }
  // <Z_c> from the diagonal, fixed-order block reduction (dm_kernel's, operation for operation)
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

// Re sum_i conj(l_i) (Gen v)_i on one quad (index a + 2 b: v0 = rho_00, v1 = rho_10, v2 = rho_01, v3 = rho_11),
// Gen v = -(i / 2) [P, v]:
//   X: -(i / 2) (v1 - v2, v0 - v3, v3 - v0, v2 - v1)     Y: (1 / 2) (-(v1 + v2), v0 - v3, v0 - v3, v1 + v2)
//   Z: (0, i v1, -i v2, 0)   (rz and p)
__device__ __forceinline__ float gen_dot(int kind, const float2 l[4], float2 v0, float2 v1, float2 v2, float2 v3) {
  if (kind == K_RX) {
    const float2 A = make_float2(v1.x - v2.x, v1.y - v2.y), B = make_float2(v0.x - v3.x, v0.y - v3.y);
    const float2 p = make_float2(l[0].x - l[3].x, l[0].y - l[3].y), q = make_float2(l[1].x - l[2].x, l[1].y - l[2].y);
    return 0.5f * ((p.x * A.y - p.y * A.x) + (q.x * B.y - q.y * B.x));
  }
  if (kind == K_RY) {
    const float2 A = make_float2(v1.x + v2.x, v1.y + v2.y), B = make_float2(v0.x - v3.x, v0.y - v3.y);
    const float2 p = make_float2(l[3].x - l[0].x, l[3].y - l[0].y), q = make_float2(l[1].x + l[2].x, l[1].y + l[2].y);
    return 0.5f * ((p.x * A.x + p.y * A.y) + (q.x * B.x + q.y * B.y));
  }
  return (l[1].y * v1.x - l[1].x * v1.y) + (l[2].x * v2.y - l[2].y * v2.x);
}

// lam <- T^dagger lam on every quad of bits (q, q + n) (apply_superop's quad walk with the conjugate transpose);
// with rho (the taped rho_{g-1}) also this thread's share of Re <T^dagger lam, Gen rho>, the tape read once
__device__ float pull_back(float2* lam, int n, int q, const float2* T, const float2* rho, int kind) {
  const int nb = 2 * n;
  const long nq = 1L << (nb - 2);
  const long lo_a = (1L << q) - 1, lo_b = (1L << (q + n)) - 1;
  float2 t[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) t[e] = conj2(T[(e & 3) * 4 + (e >> 2)]);
  float part = 0.f;
  for (long j = threadIdx.x; j < nq; j += NT) {
    long x = ((j & ~lo_a) << 1) | (j & lo_a);
    x = ((x & ~lo_b) << 1) | (x & lo_b);
    const long i0 = x, i1 = x | (1L << q), i2 = x | (1L << (q + n)), i3 = i1 | (1L << (q + n));
    const float2 v0 = lam[i0], v1 = lam[i1], v2 = lam[i2], v3 = lam[i3];
    float2 o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      o[r] = cadd(cadd(cmul(t[4 * r], v0), cmul(t[4 * r + 1], v1)), cadd(cmul(t[4 * r + 2], v2), cmul(t[4 * r + 3], v3)));
    lam[i0] = o[0];
    lam[i1] = o[1];
    lam[i2] = o[2];
    lam[i3] = o[3];
    if (rho) part += gen_dot(kind, o, rho[i0], rho[i1], rho[i2], rho[i3]);
  }
  return part;
}

// workgroup sum in a fixed order: xor butterfly within each wave, then waves 0 .. NT / 64 - 1 through LDS
__device__ float block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < NT / 64; ++w) r += red[w];
  __syncthreads();                             // red is written again at the next taped gate
  return r;
}

__global__ void __launch_bounds__(NT) dm_adjoint_kernel(AdjArgs a) {
  __shared__ float2 lam_s[1 << (2 * LDS_QUBITS)];
  __shared__ float2 T[16];
  __shared__ float red[NT / 64];
  __shared__ float wz[CMAX];
  const int s = blockIdx.x, n = a.n;
  const long N = 1L << (2 * n), D = 1L << n;
  float2* lam = n <= LDS_QUBITS ? lam_s : a.lam + (size_t)s * N;
  const float* row = a.rows + (size_t)s * a.W;
  if (threadIdx.x < a.C) wz[threadIdx.x] = a.w[(size_t)s * a.C + threadIdx.x];
  __syncthreads();
  // seed: Lambda[r, r] = sum_c w_c (1 - 2 r_c)
  for (long i = threadIdx.x; i < N; i += NT) {
    const long r = i & (D - 1);
    float v = 0.f;
    if (r == (i >> n))
      for (int c = 0; c < a.C; ++c) v += ((r >> a.readout[c]) & 1) ? -wz[c] : wz[c];
    lam[i] = make_float2(v, 0.f);
  }
  int j = 0;                                   // taped gates of the program: gate g's tape index is counted down
  for (int gi = 0; gi < a.G; ++gi) j += taped(a.gates[gi], a.n_grad) ? 1 : 0;
  __syncthreads();
  for (int gi = a.G - 1; gi >= 0; --gi) {
    const Gate g = a.gates[gi];
    float grad = 0.f;
    if (g.kind == K_CX || g.kind == K_CZ || g.kind == K_SWAP) {
      if (a.S) {                               // S^dagger on both qubits, in reverse order, before the permutation
        const float2 id[4] = {make_float2(1.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(1.f, 0.f)};
        build_superop(id, a.S, T);
        __syncthreads();
        pull_back(lam, n, g.q1, T, nullptr, 0);
        __syncthreads();
        pull_back(lam, n, g.q0, T, nullptr, 0);
        __syncthreads();
      }
      if (g.kind == K_CZ) {                    // cx, cz, swap are their own inverses
        apply_cz(lam, n, g.q0, g.q1);
      } else {
        permute_side(lam, n, g.kind, g.q0, g.q1, n);
        __syncthreads();
        permute_side(lam, n, g.kind, g.q0, g.q1, 0);
      }
    } else {
      float2 u[4];
      gate_matrix(g, row, u);
      build_superop(u, a.S, T);
      __syncthreads();
      const float2* rho = nullptr;
      if (taped(g, a.n_grad)) {
        --j;
        if (j < a.J) rho = a.tape + ((size_t)s * a.J + j) * N;
      }
      const float part = pull_back(lam, n, g.q0, T, rho, g.kind);
      if (rho) grad = block_sum(part, red);    // uniform over the workgroup
    }
    __syncthreads();
    if (threadIdx.x == 0) a.gg[(size_t)s * a.G + gi] = grad;
  }
}

}  // namespace dm

// Forward sweep with tape: <Z_c> as qfx_dm_run, and rho in front of every differentiated gate into tape [S][J][4^n]
extern "C" int qfx_dm_forward_tape(const void* gates, int G, int n, const float* rows, int W, long S, const int* readout,
                                   int C, const float* superop, void* scratch, int n_grad, int J, void* tape,
                                   float* expz, hipStream_t st) {
  if (n < 1 || n > dm::MAXQ || C < 1 || C > dm::CMAX || S <= 0 || G < 0) return (int)hipErrorInvalidValue;
  if (n > dm::LDS_QUBITS && !scratch) return (int)hipErrorInvalidValue;
  if (n_grad < 0 || n_grad > W || J < 0 || (J > 0 && !tape)) return (int)hipErrorInvalidValue;
  dm::TapeArgs a{(const dm::Gate*)gates, G, n, rows, W, readout, C, superop, (float2*)scratch, n_grad, J,
                 (float2*)tape, expz};
  hipLaunchKernelGGL(dm::dm_tape_kernel, dim3((unsigned)S), dim3(dm::NT), 0, st, a);
  return (int)hipGetLastError();
}

// Backward sweep: gg [S][G] = d(sum_c w_c <Z_c>)/d(angle of gate g) from the tape of qfx_dm_forward_tape
extern "C" int qfx_dm_adjoint(const void* gates, int G, int n, const float* rows, int W, long S, const int* readout, int C,
                              const float* superop, int n_grad, int J, const void* tape, void* lam, const float* w,
                              float* gg, hipStream_t st) {
  if (n < 1 || n > dm::MAXQ || C < 1 || C > dm::CMAX || S <= 0 || G < 0) return (int)hipErrorInvalidValue;
  if (n > dm::LDS_QUBITS && !lam) return (int)hipErrorInvalidValue;
  if (n_grad < 0 || n_grad > W || J < 0 || (J > 0 && !tape)) return (int)hipErrorInvalidValue;
  if (G == 0) return (int)hipSuccess;
  dm::AdjArgs a{(const dm::Gate*)gates, G, n, rows, W, readout, C, superop, n_grad, J, (const float2*)tape,
                (float2*)lam, w, gg};
  hipLaunchKernelGGL(dm::dm_adjoint_kernel, dim3((unsigned)S), dim3(dm::NT), 0, st, a);
  return (int)hipGetLastError();
}
