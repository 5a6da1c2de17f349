"""Shared case table of the tile-shape tests of the generic (VALU) statevector engine.

The pass kernels (``csrc/statevec.hip`` interpreter, ``csrc/jit.cpp`` per-plan kernels) change shape with the tile
size k = min(n, kmax): T = 2^(k - log2 R) threads own a tile and 256 / T tiles share a workgroup.  ``HipProgram(kmax=)``
forces small tiles, so every T from 1 to 256 - with qubits outside the tile - runs at 3..14 qubits.  The CPU twin
(``test_statevec_tiles.py``) holds the plans of every case to float64 through the register-level emulator and proves
which plan features each case reaches; the GPU twin (``test_gpu_statevec_tiles.py``) runs the same cases on both kernels.

Every case runs K = 3 parameter rows x B = 3 samples (S = 9, spc = 3): workgroups straddle samples and theta rows and
the last workgroup is partly invalid.  Slot map: ``theta`` at 0, ``x`` after it; ``x`` carries one encoding angle per
qubit and, past those, the per-sample selectors (0..3 = I/X/Y/Z) of the ``pauli`` gates.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from qfedx_amd.ops.plan_tools import (FIN_READOUT, INIT_PSI_LAMBDA, K_PAULI, OP_CX, OP_CZ, OP_D1T, OP_G1, OP_REMAP,
                                      PHYS_NONTILE)
from qfedx_amd.ops.statevec_torch import TorchProgram, slot_grads
from qfedx_amd.quantum.circuit import Circuit, ParameterVector

K_ROWS, B_SAMPLES = 3, 3
S_SAMPLES = K_ROWS * B_SAMPLES
MODES = {"fwd": (0, 3), "load": (1, 3), "adj": (2, 0)}      # name -> (planner mode, final flags)


@dataclass(frozen=True)
class Case:
    name: str
    n: int
    kmax: int
    R: int
    build: Callable[[], Circuit]
    n_theta: int
    x_width: int
    readout: tuple
    features: frozenset        # "<mode>/<feature>" strings that plan_features must report for this case
    jit: bool                  # also runs on the per-plan (hiprtc) kernels; every case runs on the interpreter

    @property
    def slots(self) -> dict:
        return {"theta": 0, "x": self.n_theta}

    def program(self):
        return self.build().to_program(self.slots)


# ------------------------------------------------------------------------------------------------ plan features
def _cls(p: int, rb: int) -> str:
    return "reg" if p < rb else "thr" if p < PHYS_NONTILE else "non"


def plan_features(info: dict, rb: int) -> set:
    """Feature strings of one plan (``parse_blob`` output): which operand bit classes (register / thread / non-tile)
    every micro-op kind, the readout and the lambda seed act on, the G1 group lengths, pass count and pass modes.
    ``PAULI:<cls>`` is the class of a trajectory Pauli's qubit when its pass starts; ``non`` = outside the tile of
    the pass before (a Pauli needs a register bit, so the planner must bring that qubit into the tile)."""
    f = {f"PASSES:{info['npass']}"} | ({"MULTIPASS"} if info["npass"] > 1 else set())
    prev_nontile: set = set()
    for p in info["passes"]:
        f |= {f"INIT:{p['INIT']}", f"FINAL:{p['FINAL']}"}
        for op in p["ops"]:
            a, b = op["a"], op["b"]
            if op["code"] == OP_D1T:
                f.add(f"D1T:{_cls(a, rb)}")
            elif op["code"] == OP_CX:
                f.add(f"CX:{_cls(a, rb)}")
            elif op["code"] == OP_CZ:
                f.add("CZ:" + "-".join(sorted((_cls(a, rb), _cls(b, rb)))))
            elif op["code"] == OP_REMAP:
                f.add("REMAP")
            elif op["code"] == OP_G1:
                f.add(f"G1:{len(op['gates'])}")
                for gi in op["gates"]:
                    g = info["gates"][gi]
                    if g["kind"] == K_PAULI:
                        q = g["q0"]
                        f.add("PAULI:" + ("non" if q in prev_nontile else _cls(p["q0"].index(q), rb)))
        if p["FINAL"] & FIN_READOUT:
            f |= {f"READ:{_cls(ph, rb)}" for ph in p["read_phys"]}
        if p["INIT"] == INIT_PSI_LAMBDA:
            f |= {f"LAM:{_cls(ph, rb)}" for ph in p["lam_phys"]}
        prev_nontile = set(p["nontile"])
    return f


# ------------------------------------------------------------------------------------------------ circuits
_FIXED = ["h", "x", "y", "z", "s", "sdg", "t", "tdg", "sx"]


def random_circuit(n: int, n_theta: int, n_pauli: int, seed: int, gates: int) -> Circuit:
    """The seeded generator of tests/test_simulator.py, extended with ``swap``, ``pauli`` (selector slots x[n..]) and
    a leading RY(x_q) product prefix."""
    rng = np.random.default_rng(seed)
    th, x = ParameterVector("theta", n_theta), ParameterVector("x", n + n_pauli)
    qc = Circuit(n)
    for q in range(n):
        qc.ry(x[q], q)
    pauli = 0
    for i in range(gates):
        r = rng.random()
        q = int(rng.integers(n))
        if r < 0.38:
            getattr(qc, ["rx", "ry", "rz", "p"][int(rng.integers(4))])(th[i % n_theta] * float(rng.uniform(0.5, 1.5)), q)
        elif r < 0.54:
            getattr(qc, _FIXED[int(rng.integers(9))])(q)
        elif r < 0.60 and pauli < n_pauli:
            qc.pauli(x[n + pauli], q)
            pauli += 1
        else:
            a, b = (int(v) for v in rng.choice(n, 2, replace=False))
            if r < 0.80:
                qc.cx(a, b)
            elif r < 0.95:
                qc.cz(a, b)
            else:
                qc.swap(a, b)
    return qc


def directed_circuit(n: int, n_theta: int, run_qubit: int, pauli_qubits: tuple) -> Circuit:
    """Every gate kind on every qubit AFTER it is entangled (so it is planned as a micro-op, not folded into the product
    prefix), a run of 12 single-qubit gates on one entangled qubit (a forward G1 group of MAX_GROUP = 8 plus the
    overflow group), three Paulis, CX / CZ between near and far qubits in both directions, a swap, theta slots shared
    by gates far apart in the circuit and an x-slot rotation after the prefix (it carries no reported gradient)."""
    th, x = ParameterVector("theta", n_theta), ParameterVector("x", n + 3)
    qc = Circuit(n)
    t = iter(range(10 ** 6))
    nxt = lambda: th[next(t) % n_theta]                                   # noqa: E731
    for q in range(n):
        qc.ry(x[q], q)
        qc.rz(nxt() * 0.8, q)
    for q in range(n - 1):
        qc.cx(q, q + 1)
    for q in range(n):                                                  # diagonal + rotation kinds on every bit class
        qc.rx(nxt() * 1.1 + 0.1, q)
        qc.p(nxt() * 0.9, q)
        getattr(qc, _FIXED[q % 9])(q)
    for a in range(n):                                                  # CZ in every class pair, CX from every control
        qc.cz(a, (a + 1) % n)
        qc.cz(a, (a + n // 2) % n)
        if a % 2 == 0:
            qc.cx((a + n // 2) % n, a)
    q = run_qubit
    for j, g in enumerate(["rx", "h", "ry", "sx", "rz", "rx", "y", "p", "ry", "sdg", "rx", "ry"]):
        if g in ("rx", "ry", "rz", "p"):
            getattr(qc, g)(nxt() * (0.6 + 0.05 * j), q)
        else:
            getattr(qc, g)(q)
    for j, pq in enumerate(pauli_qubits):
        qc.pauli(x[n + j], pq)
        qc.cx(pq, (pq + 1) % n)
    qc.swap(0, n - 1)
    qc.rx(x[0] * 0.7, n // 2)                                           # x-slot rotation after the prefix
    for q in range(n):
        (qc.ry if q % 2 == 0 else qc.rz)(nxt() * 0.5 + (-0.2), q)
    for a in range(n):                                                  # partners in other tiles: the diagonal gates
        qc.cz(a, (a + n // 2) % n)                                      # behind them run on non-tile qubits
    for a in range(0, n - 1, 2):
        qc.cz(a, a + 1)
    for q in range(n):
        qc.p(nxt() * 0.3, q)
    qc.rz(th[0] * 1.3, n - 1)                                          # slot 0 again, far from its first use
    qc.rx(th[1] * 0.4, 0)
    return qc


# ------------------------------------------------------------------------------------------------ the grid
def _rand(n, n_theta, n_pauli, seed, gates=36):
    return functools.partial(random_circuit, n, n_theta, n_pauli, seed, gates)


def _case(name, n, kmax, build, n_theta, n_pauli, readout, features, jit, R=16):
    return Case(name, n, kmax, R, build, n_theta, n + n_pauli, tuple(readout), frozenset(features.split()), jit)


_DIRECTED = ("fwd/G1:8 fwd/D1T:thr fwd/D1T:non fwd/CX:reg fwd/CX:thr fwd/CX:non fwd/PAULI:reg fwd/PAULI:thr "
             "fwd/PAULI:non fwd/REMAP fwd/MULTIPASS fwd/INIT:0 load/MULTIPASS load/G1:8 adj/G1:8 adj/D1T:thr "
             "adj/D1T:non adj/CX:reg adj/CX:thr adj/CX:non adj/CZ:thr-thr adj/INIT:3 adj/REMAP ")

# name, n, kmax, circuit, n_theta, Pauli slots, readout, claimed plan features, runs on the per-plan kernels too
CASES = [
    # T = 1 (256 tiles / block), R = 4 kernels with a non-tile qubit
    _case("r4_3q_k2", 3, 2, _rand(3, 4, 1, 3, 24), 4, 1, [0, 2],
          "fwd/CX:non fwd/CZ:non-reg fwd/READ:non load/MULTIPASS adj/CX:non adj/LAM:non adj/INIT:3", False, R=4),
    # T = 1: no thread bits at all
    _case("rand_6q_k4", 6, 4, _rand(6, 6, 2, 6), 6, 2, [0, 3, 5],
          "fwd/CX:non fwd/CZ:non-reg fwd/READ:non fwd/MULTIPASS load/MULTIPASS adj/CZ:non-non adj/D1T:non "
          "adj/LAM:non adj/INIT:3", True),
    # T = 2: smallest group_sum
    _case("rand_7q_k5", 7, 5, _rand(7, 6, 2, 7), 6, 2, [0, 6],
          "fwd/CX:thr fwd/CX:non fwd/D1T:thr fwd/READ:thr fwd/READ:non fwd/REMAP load/CZ:non-thr adj/D1T:non "
          "adj/LAM:thr adj/REMAP", False),
    # T = 4: sub-wave, second block mostly invalid
    _case("rand_9q_k6", 9, 6, _rand(9, 6, 2, 9), 6, 2, [0, 4, 8],
          "fwd/CZ:non-non fwd/CZ:non-thr fwd/READ:reg fwd/READ:thr fwd/READ:non adj/CX:thr adj/D1T:non adj/D1T:thr",
          False),
    _case("dir_9q_k6", 9, 6, functools.partial(directed_circuit, 9, 7, 3, (1, 5, 8)), 7, 3, [0, 1, 2, 3, 4, 5, 6, 8],
          _DIRECTED + "fwd/CZ:non-reg fwd/CZ:non-thr fwd/CZ:reg-reg fwd/CZ:reg-thr fwd/CZ:thr-thr fwd/READ:reg "
          "fwd/READ:thr fwd/READ:non adj/CZ:non-non adj/CZ:non-reg adj/CZ:non-thr adj/CZ:reg-reg adj/CZ:reg-thr "
          "adj/LAM:reg adj/LAM:thr adj/LAM:non adj/PAULI:non", True),
    # T = 8: k = 7
    _case("rand_10q_k7", 10, 7, _rand(10, 6, 2, 10), 6, 2, [0, 5, 9],
          "fwd/CZ:thr-thr fwd/CX:thr fwd/READ:non load/MULTIPASS adj/D1T:non adj/LAM:thr adj/INIT:3", False),
    # T = 16: one DPP row per tile
    _case("rand_11q_k8", 11, 8, _rand(11, 6, 2, 11), 6, 2, [1, 10],
          "fwd/D1T:non fwd/CX:non fwd/CZ:non-thr load/READ:non adj/CZ:non-thr adj/D1T:non adj/INIT:3", False),
    # T = 64: table (use_tab) workgroup of 4 tiles = two samples, whose theta rows differ at every third sample
    _case("rand_11q_k10", 11, 10, _rand(11, 6, 2, 12), 6, 2, [0, 10],
          "fwd/CX:non fwd/CZ:non-thr fwd/CZ:non-reg load/MULTIPASS adj/CX:non adj/CZ:non-reg adj/CZ:non-thr", True),
    # T = 64 with two non-tile qubits
    _case("rand_12q_k10", 12, 10, _rand(12, 6, 2, 13), 6, 2, [0, 6, 11],
          "fwd/CZ:non-reg fwd/READ:non load/CZ:non-thr load/MULTIPASS adj/LAM:non adj/CZ:non-reg adj/INIT:3", False),
    _case("dir_12q_k10", 12, 10, functools.partial(directed_circuit, 12, 7, 4, (2, 7, 11)), 7, 3, [9],
          _DIRECTED + "fwd/CZ:non-non fwd/CZ:non-thr fwd/CZ:reg-reg fwd/CZ:reg-thr fwd/CZ:thr-thr adj/CZ:non-reg "
          "adj/CZ:non-thr adj/LAM:non", True),
    # T = 128: cross-wave sums, two tiles per block
    _case("rand_13q_k11", 13, 11, _rand(13, 6, 2, 14), 6, 2, [0, 7, 12],
          "fwd/CX:non fwd/CZ:non-thr fwd/CZ:non-reg fwd/READ:non load/MULTIPASS adj/D1T:non adj/LAM:non "
          "adj/CZ:non-reg", True),
    # T = 256: the production tile on a generic circuit, both kernels
    _case("rand_14q_k12", 14, 12, _rand(14, 6, 2, 15), 6, 2, [0, 7, 13],
          "fwd/CX:non fwd/CZ:non-reg fwd/READ:non load/MULTIPASS adj/D1T:non adj/LAM:non adj/CX:non", True),
]
# bf16 storage between passes (per-plan kernels only): every pass boundary rounds the state
BF16_CASE = _case("dir_10q_k7_bf16", 10, 7, functools.partial(directed_circuit, 10, 7, 3, (1, 5, 9)), 7, 3, [0, 4, 9],
                  "fwd/MULTIPASS fwd/D1T:non fwd/READ:non fwd/G1:8 adj/MULTIPASS adj/LAM:non adj/CZ:non-non", True)
BY_NAME = {c.name: c for c in CASES + [BF16_CASE]}

# what the union of the cases must reach, on the interpreter and again on the per-plan kernels
_OPS = ["D1T:thr", "D1T:non", "CX:reg", "CX:thr", "CX:non", "REMAP", "G1:8", "MULTIPASS"] + \
       ["CZ:" + p for p in ("reg-reg", "reg-thr", "non-reg", "thr-thr", "non-thr", "non-non")]
REQUIRED = frozenset([f"fwd/{f}" for f in _OPS + ["READ:reg", "READ:thr", "READ:non", "PAULI:reg", "PAULI:thr",
                                                   "PAULI:non", "INIT:0", "INIT:1"]] +
                     [f"adj/{f}" for f in _OPS + ["LAM:reg", "LAM:thr", "LAM:non", "INIT:2", "INIT:3"]] +
                     ["load/MULTIPASS", "load/INIT:0", "load/G1:8", "load/D1T:non", "load/CX:non", "load/CZ:non-non",
                      "load/READ:non"])


# ------------------------------------------------------------------------------------------------ inputs, references
@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """Deterministic float32 inputs of a case: theta [K, n_theta], x [K, B, x_width] (angles, then Pauli selectors
    which take every value on every Pauli gate across the samples), readout weights w [S, C], a complex normalised
    initial state per sample and real raw rows with F < 2^n columns, one of them all-zero (-> the uniform state)."""
    c = BY_NAME[name]
    rng = np.random.default_rng(sum(name.encode()))
    K, B, S, N = K_ROWS, B_SAMPLES, S_SAMPLES, 1 << c.n
    x = rng.uniform(0, 3, (S, c.x_width))
    for j in range(c.x_width - c.n):
        col = np.arange(S) + j
        x[:, c.n + j] = 1 + col % 3 if name.startswith("dir") else col % 4   # directed: selectors 1, 2, 3 only
    init_c = rng.normal(size=(S, N)) + 1j * rng.normal(size=(S, N))
    init_c /= np.linalg.norm(init_c, axis=1, keepdims=True)
    F = N - 3 if N > 8 else N - 1
    init_r = rng.normal(size=(S, F))
    init_r[4] = 0.0
    return dict(theta=torch.tensor(rng.normal(size=(K, c.n_theta)), dtype=torch.float32),
                x=torch.tensor(x, dtype=torch.float32).reshape(K, B, c.x_width),
                w=torch.tensor(rng.normal(size=(S, len(c.readout))), dtype=torch.float32),
                init_c=torch.tensor(init_c, dtype=torch.complex64), init_r=torch.tensor(init_r, dtype=torch.float32))


def rows_of(name: str, dtype=torch.float64) -> torch.Tensor:
    """[S, n_theta + x_width] slot values of every sample (sample s uses theta row s // B)."""
    i = inputs(name)
    return torch.cat([i["theta"].repeat_interleave(B_SAMPLES, 0), i["x"].reshape(S_SAMPLES, -1)], 1).to(dtype)


def start_states(name: str, dtype=torch.complex128) -> dict:
    """start name -> initial states [S, 2^n] (None = |0..0>): the float32 inputs, encoded in float64."""
    c, i = BY_NAME[name], inputs(name)
    N = 1 << c.n
    raw = torch.zeros(S_SAMPLES, N, dtype=torch.float64)
    raw[:, : i["init_r"].shape[1]] = i["init_r"].double()
    nrm = raw.norm(dim=1, keepdim=True)
    amp = torch.where(nrm > 0, raw / nrm.clamp_min(1e-300), torch.full_like(raw, N ** -0.5))
    return {"prod": None, "cplx": i["init_c"].to(dtype), "real": amp.to(dtype)}


def _run(name: str, dtype) -> dict:
    c, i = BY_NAME[name], inputs(name)
    ops, coef = c.program()
    prog = TorchProgram(ops, coef, c.n, dtype=dtype)
    rows = rows_of(name, prog.rdtype)
    out = {}
    for start, init in start_states(name, dtype).items():
        psi = prog.run(rows, state=init)
        z = prog.expz(psi, list(c.readout))
        gg = prog.adjoint_grads(rows, psi, i["w"].to(prog.rdtype), list(c.readout))
        g = slot_grads(gg, torch.from_numpy(ops), torch.from_numpy(coef), c.n_theta + c.x_width)[:, : c.n_theta]
        out[start] = dict(psi=psi, z=z, grad=g.reshape(K_ROWS, B_SAMPLES, c.n_theta).sum(1), grad_s=g)
    return out


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """float64 reference (``TorchProgram(complex128)``, CPU) of a case: start -> final states [S, 2^n], <Z> [S, C] and
    d/dtheta of sum_c w <Z_c> per sample (``grad_s`` [S, n_theta]) and summed over the B samples of each parameter
    row (``grad`` [K, n_theta]).  Computed once per case and shared read-only by the tests."""
    return _run(name, torch.complex128)


def max_errors(got: dict, ref: dict) -> dict:
    return {k: float((got[k].detach().cpu().to(ref[k].dtype) - ref[k]).abs().max()) for k in got}


@functools.lru_cache(maxsize=None)
def executor_errors(name: str) -> dict:
    """Yardstick: the fp32 torch executor's own maximum error against the float64 reference, per start."""
    ref = reference(name)
    return {start: max_errors(r, ref[start]) for start, r in _run(name, torch.complex64).items()}

