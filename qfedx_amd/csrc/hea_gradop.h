// Per-gradient-op formulas of the MFMA engine's gradient reductions (hea_step.hip hea_grad_reduce_kernel, hea_dpsgd.hip):
// the 32 partial-trace sums of one gradient op -> (d/dtheta, d/dphi) of each of its real qubits.
#pragma once
#include <hip/hip_runtime.h>

namespace qfx {

// Real qubit j of gradient record m (gmeta row: m[1] bit 4 = inside, m[2 + j] / m[6 + j] = the theta / phi parameter)
// from the op's summed partial traces pt[32] (slots 8j + 4y + 2x + comp = n_j[y][x].(re, im)), with the client's
// parameter row prm:
//   outside:  d/dtheta = Im(e^{-i phi} n10 + e^{i phi} n01),   d/dphi = Im(n00 - n11)
//   inside (cross matrix taken at the op INPUT, transposed BACK ops):
//             d/dtheta = Im<lam|X|psi> = Im(n01 + n10);
//             d/dphi = Im<lam|RX^H Z RX|psi> = cos(theta) Im(n00 - n11) + sin(theta) Re(n01 - n10)
// Results in double: the callers round them (hea_grad_reduce: to float, bitwise what it always wrote).
__device__ inline void hea_gradop_pair(const double* pt, const float* prm, const int* m, int j, int inside, double& gth,
                                       double& gph) {
  const double* p = pt + 8 * j;
  if (inside) {
    const double th = prm[m[2 + j]];
    const double ct = cos(th), st = sin(th);
    gth = p[3] + p[5];
    gph = ct * (p[1] - p[7]) + st * (p[2] - p[4]);
  } else {
    const double ph = prm[m[6 + j]];
    const double cp = cos(ph), sp = sin(ph);
    gth = (cp * p[5] - sp * p[4]) + (cp * p[3] + sp * p[2]);
    gph = p[1] - p[7];
  }
}

}  // namespace qfx
