"""Programs, inputs and the float64 oracle shared by tests/test_density_adjoint.py (CPU), tests/
test_gpu_density_adjoint.py and tools/density_adjoint_err_table.py.

The oracle is the gate-level +-pi/2 shift rule evaluated in float64 through the simulator's long-standing forward
pass ``DensityProgram._expz_torch`` (never through ``_vjp_torch``): exact for rx / ry / rz / p with
parameter-independent channels in between.
"""
import functools
import math

import numpy as np
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops.density import DensityProgram, kraus_ops
from qfedx_amd.quantum.circuit import KIND


def shifted(prog: DensityProgram, g: int, delta: float, device="cpu") -> DensityProgram:
    """``prog`` with ``delta`` added to the angle of gate g (its offset), same channel."""
    coef = prog.coef.astype(np.float64).copy()
    coef[g, 1] += delta
    sh = DensityProgram(prog.ops, coef, prog.n, prog.readout, device)
    sh.S = prog.S
    if torch.device(device).type == "cuda":
        sh._sup = prog._sup
    return sh


def oracle(prog: DensityProgram, rows: torch.Tensor, w: torch.Tensor, n_grad: int):
    """float64 (<Z> [S, C], gg [S, G]) of sum_c w_c <Z_c>."""
    rows, w = rows.double().cpu(), w.double().cpu()
    gg = torch.zeros(rows.shape[0], len(prog.ops), dtype=torch.float64)
    for g in prog.taped_gates(n_grad):
        zp, zm = (shifted(prog, g, s * math.pi / 2)._expz_torch(rows) for s in (1.0, -1.0))
        gg[:, g] = 0.5 * ((zp - zm) * w).sum(-1)
    return prog._expz_torch(rows), gg


def vqc_case(n, L, kind, p, gamma, entangler, readout, S=3, device="cpu"):
    """(program, rows [S, W] float32, w [S, C] float32, n_grad) of the hardware-efficient VQC."""
    spec = VQCSpec(n, L, 2, init_std=1.0, entangler=entangler)
    ops, coef = spec.program()
    kr = kraus_ops(kind, p, gamma) if kind != "none" else None
    prog = DensityProgram(ops, coef, n, readout, device, kraus=kr)
    g = torch.Generator().manual_seed(100 * n + L)
    rows = torch.cat([torch.randn(S, spec.n_theta, generator=g), torch.rand(S, n, generator=g) * 3], -1)
    w = torch.randn(S, len(readout), generator=g)
    return prog, rows, w, spec.n_theta


def hand_case(S=3, device="cpu"):
    """A 3-qubit program with every gate kind of the kernel: a fixed gate, all four rotations, a slot used twice, a
    scaled and offset angle, all three two-qubit gates, and a parametrised gate outside [0, n_grad)."""
    K = KIND                                             # records written out: Circuit lowers swap to three cx
    prog = [("h", 0, -1, -1, 0.0, 0.0), ("rx", 0, -1, 0, 1.0, 0.0), ("cz", 0, 2, -1, 0.0, 0.0),
            ("ry", 1, -1, 1, 2.0, 0.3), ("swap", 1, 2, -1, 0.0, 0.0), ("p", 2, -1, 0, 1.0, 0.0),
            ("rz", 1, -1, 2, 1.0, 0.0), ("cx", 2, 0, -1, 0.0, 0.0), ("rx", 0, -1, 3, 1.0, 0.0)]
    ops = np.array([(K[g[0]], *g[1:4]) for g in prog], np.int32)
    coef = np.array([g[4:] for g in prog], np.float32)
    prog = DensityProgram(ops, coef, 3, [0, 2], device, kraus=kraus_ops("amplitude", gamma=0.15))
    g = torch.Generator().manual_seed(7)
    return prog, torch.randn(S, 4, generator=g), torch.randn(S, 2, generator=g), 3


# The GPU cases: the smallest shapes at which the kernels change branch (S = 3 rows each).
GPU_CASES = {
    "n2": lambda dev: vqc_case(2, 1, "amplitude", 0.0, 0.2, "chain", [0, 1], device=dev),         # 4 quads < one wave
    "n4_ring_dep": lambda dev: vqc_case(4, 2, "depolarizing", 0.05, 0.0, "ring", [0, 3, 1], device=dev),
    "n6": lambda dev: vqc_case(6, 2, "amplitude", 0.0, 0.1, "chain", [0, 5, 2], device=dev),      # the LDS limit
    "n7": lambda dev: vqc_case(7, 2, "amplitude", 0.0, 0.05, "chain", [0, 3, 6], device=dev),     # first global slab
    "n8_ideal": lambda dev: vqc_case(8, 1, "none", 0.0, 0.0, "chain", [0, 7], device=dev),        # S null
    "hand": lambda dev: hand_case(device=dev),
}


@functools.lru_cache(maxsize=None)
def gpu_case_oracle(name: str):
    """The float64 oracle of a GPU case, computed once per process."""
    prog, rows, w, n_grad = GPU_CASES[name]("cpu")
    return oracle(prog, rows, w, n_grad)
