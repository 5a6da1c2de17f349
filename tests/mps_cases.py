"""Shared case table of the shape-edge tests of the two MPS kernels.

``csrc/mps_chain.hip`` (one wave per sample, bond <= 8) and ``csrc/mps_mpo.hip`` (one 256-thread workgroup per sample,
bond <= 16) are index arithmetic over boundary columns, pass-through masks, event bit fields and per-wave reductions.
This module keeps the directed cases that reach their edges, the seeded float32 inputs and the float64 references in
one place.  The CPU twin (``test_mps_cases.py``) proves from the compiled tables what each case reaches and holds the
references to the complex128 dense statevector; the GPU twin (``test_gpu_mps_edges.py``) runs the same cases on the
kernels.

Chain cases are ``VQCSpec`` shapes with a batch shape (K clients x B samples); angles (features and theta) are uniform
in [-7, 7], several periods wide.  MPO cases are circuits lowered with ``Circuit.to_program`` and run on their float32
gate-angle table [S, G] - that table IS the input, the references read it in float64 through an identity-slot copy of
the program (every gate its own slot), so no fp32 slot arithmetic sits between the kernel's input and the reference's.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops.engine import ce_readout
from qfedx_amd.ops.statevec_torch import TorchProgram, gate_angles, slot_grads
from qfedx_amd.quantum.circuit import Circuit, ParameterVector
from qfedx_amd.quantum.mps_chain import chain_columns
from qfedx_amd.quantum.mps_mpo import ROTATIONS, compile_mpo

# bounds of the kernels against float64: the project's existing ones (tests/test_gpu_mps_chain.py, tests/test_gpu_mps.py)
TOL = dict(z=2e-5, dang=5e-5, grad=1e-4, fused_grad=1e-4, dl=2e-5, loss_rtol=1e-4, loss_atol=1e-5, sim_grad=5e-5)
ANGLE = 7.0
BATCHES = ((1, 1), (3, 3), (2, 5), (5, 1))       # (3, 3): two clients' theta rows in one block, last block one wave


# ------------------------------------------------------------------------------------------------ chain cases
@dataclass(frozen=True)
class ChainCase:
    name: str
    n: int
    L: int
    feature: str
    readout: tuple
    K: int = 3
    B: int = 3
    variant: str = ""          # "rows": theta passed as full parameter rows; "xpad": x with n + 3 columns, NaN behind n

    @property
    def C(self) -> int:
        return len(self.readout)

    @property
    def S(self) -> int:
        return self.K * self.B

    def spec(self) -> VQCSpec:
        return VQCSpec(self.n, self.L, self.C, feature_map=self.feature, readout=list(self.readout))


_RO_N2_C8 = (0, 1, 0, 1, 1, 0, 0, 1)
_RO_N10_C8 = (9, 0, 3, 3, 7, 1, 8, 2)


def _chain_cases() -> list:
    out = [ChainCase("n2_L1_ro11", 2, 1, "ry", (1, 1)),
           ChainCase("n2_L1_ro00", 2, 1, "ry", (0, 0)),                        # qmax = 0
           ChainCase("n3_L2_rz_ro00", 3, 2, "rz", (0, 0)),
           ChainCase("n3_L3_ry_ro10", 3, 3, "ry", (1, 0))]
    out += [ChainCase(f"n4_L{L}_{f}", 4, L, f, (0, 1, 2)) for L in (1, 2, 3) for f in ("ry", "rx", "rz")]
    for K, B in BATCHES:
        out += [ChainCase(f"n2_L3_c8_k{K}b{B}", 2, 3, "ry", _RO_N2_C8, K, B),
                ChainCase(f"n10_L3_rz_c8_k{K}b{B}", 10, 3, "rz", _RO_N10_C8, K, B),
                ChainCase(f"n10_L2_rx_ro210_k{K}b{B}", 10, 2, "rx", (2, 1, 0), K, B)]   # RO sweep starts mid-chain
    out += [ChainCase("n10_L2_rx_rows", 10, 2, "rx", (2, 1, 0), 3, 3, "rows"),
            ChainCase("n3_L3_ry_xpad", 3, 3, "ry", (1, 0), 3, 3, "xpad")]
    return out


CHAIN_CASES = _chain_cases()
# fused one-launch training step (MpsChainProgram.train): K = 3 clients x B = 3 samples
FUSED_CASES = [ChainCase("fused_n2_L3_c8", 2, 3, "ry", _RO_N2_C8),
               ChainCase("fused_n10_L3_c8", 10, 3, "rz", _RO_N10_C8),
               ChainCase("fused_n5_L2_c2", 5, 2, "ry", (0, 1))]
CHAIN_BY_NAME = {c.name: c for c in CHAIN_CASES + FUSED_CASES}
LOGIT_GAP = 1e-3


def _seed(name: str) -> int:
    return sum((i + 1) * b for i, b in enumerate(name.encode()))


@functools.lru_cache(maxsize=None)
def chain_inputs(name: str) -> dict:
    """Seeded float32 inputs: x [K, B, n] and theta [K, n_theta] uniform in [-7, 7], w [K, B, C] normal / sqrt(C);
    ``xarg`` / ``targ`` are what the kernel wrapper is called with (the call-shape variants widen them).  Fused cases
    add params [K, n_theta + 2 C] (theta | a of mixed sign | nonzero b), labels y and loss weights with exact zeros."""
    c = CHAIN_BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    nt = 2 * c.n * c.L
    x = torch.tensor(rng.uniform(-ANGLE, ANGLE, (c.K, c.B, c.n)), dtype=torch.float32)
    theta = torch.tensor(rng.uniform(-ANGLE, ANGLE, (c.K, nt)), dtype=torch.float32)
    w = torch.tensor(rng.normal(size=(c.K, c.B, c.C)) / np.sqrt(c.C), dtype=torch.float32)
    out = dict(x=x, theta=theta, w=w, xarg=x, targ=theta)
    if c.variant == "rows":
        out["targ"] = torch.cat([theta, torch.tensor(rng.normal(size=(c.K, 2 * c.C)), dtype=torch.float32)], 1)
    if c.variant == "xpad":
        out["xarg"] = torch.cat([x, torch.full((c.K, c.B, 3), float("nan"))], -1)
    if name.startswith("fused"):
        a = rng.normal(size=(c.K, c.C)) * 1.5
        a[:, 0], a[:, 1] = np.abs(a[:, 0]) + 0.3, -np.abs(a[:, 1]) - 0.3           # both signs in every row
        b = rng.normal(size=(c.K, c.C))
        out["params"] = torch.cat([theta, torch.tensor(a, dtype=torch.float32),
                                   torch.tensor(b, dtype=torch.float32)], 1)
        out["y_rand"] = torch.tensor(rng.integers(0, c.C, (c.K, c.B)))
        wm = rng.uniform(0.1, 1.0, (c.K, c.B))
        wm[0, 1] = wm[2, 0] = 0.0                                                   # exact zeros
        out["wmask"] = torch.tensor(wm, dtype=torch.float32)
    return out


def _chain_oracle(c: ChainCase, x: torch.Tensor, theta: torch.Tensor, w: Optional[torch.Tensor]):
    z, g = chain_columns(x.double().numpy().reshape(c.S, c.n), np.repeat(theta.double().numpy(), c.B, 0), c.n, c.L,
                         list(c.readout), c.feature, None if w is None else w.double().numpy().reshape(c.S, c.C))
    return torch.from_numpy(z), None if g is None else torch.from_numpy(g)


@functools.lru_cache(maxsize=None)
def chain_reference(name: str) -> dict:
    """float64 column oracle (``chain_columns``) on the float32 inputs: z [S, C], grad_s [S, 2 n L] and the per-client
    sums grad [K, 2 n L].  Computed once per case, shared read-only."""
    c, i = CHAIN_BY_NAME[name], chain_inputs(name)
    z, g = _chain_oracle(c, i["x"], i["theta"], i["w"])
    return dict(z=z, grad_s=g, grad=g.reshape(c.K, c.B, -1).sum(1))


def _fused_from_z(c: ChainCase, i: dict, z: torch.Tensor, y: torch.Tensor, grads_of) -> dict:
    """ce_readout on <Z> [S, C] in z's dtype, then the gradient of sum_c w_c <Z_c> with w = dL/d<Z> (``grads_of``)."""
    th, a, b = c.spec().split(i["params"].to(z.dtype))
    wm = i["wmask"].to(z.dtype)
    zk = z.reshape(c.K, c.B, c.C)
    loss, w, ga, gb, correct = ce_readout(zk, y, wm, a, b)
    logits = zk * a.unsqueeze(-2) + b.unsqueeze(-2)
    dl = (torch.softmax(logits, -1) - torch.nn.functional.one_hot(y, c.C).to(z.dtype)) * wm.unsqueeze(-1)
    gs = grads_of(w)
    grad = torch.cat([gs.reshape(c.K, c.B, -1).sum(1), ga, gb], -1)
    nll = -torch.log_softmax(logits, -1).gather(-1, y.unsqueeze(-1)).squeeze(-1)
    hitv = ((logits.argmax(-1) == y) & (wm > 0)).to(z.dtype)
    return dict(z=z, loss=loss, grad=grad, correct=correct, dl=dl.reshape(c.S, c.C), lossv=(nll * wm).reshape(c.S),
                hitv=hitv.reshape(c.S), logits=logits.reshape(c.S, c.C))


@functools.lru_cache(maxsize=None)
def fused_labels(name: str) -> torch.Tensor:
    """Labels [K, B]: the float64 argmax on every even sample (hits), a seeded draw on the odd ones."""
    c, i = CHAIN_BY_NAME[name], chain_inputs(name)
    z, _ = _chain_oracle(c, i["x"], i["theta"], None)
    _, a, b = c.spec().split(i["params"].double())
    am = (z.reshape(c.K, c.B, c.C) * a.unsqueeze(-2) + b.unsqueeze(-2)).argmax(-1)
    even = (torch.arange(c.S).reshape(c.K, c.B) % 2) == 0
    return torch.where(even, am, i["y_rand"])


@functools.lru_cache(maxsize=None)
def fused_reference(name: str) -> dict:
    """float64 fused step: ``chain_columns`` <Z> -> ``ce_readout`` -> ``chain_columns`` gradients with w = dL/d<Z>.
    loss / correct [K], grad [K, n_theta + 2 C] (theta | a | b), z / dl / logits [S, C], lossv / hitv [S]."""
    c, i = CHAIN_BY_NAME[name], chain_inputs(name)
    z, _ = _chain_oracle(c, i["x"], i["theta"], None)
    return _fused_from_z(c, i, z, fused_labels(name), lambda w: _chain_oracle(c, i["x"], i["theta"], w)[1])


def _chain_dense(c: ChainCase, i: dict, dtype):
    ops, coef = c.spec().program()
    prog = TorchProgram(ops, coef, c.n, "cpu", dtype=dtype)
    rows = torch.cat([i["theta"].repeat_interleave(c.B, 0), i["x"].reshape(c.S, c.n)], 1).to(prog.rdtype)
    psi = prog.run(rows)
    z = prog.expz(psi, list(c.readout))

    def grads_of(w):
        gg = prog.adjoint_grads(rows, psi, w.reshape(c.S, c.C).to(prog.rdtype), list(c.readout))
        return slot_grads(gg, torch.from_numpy(ops), torch.from_numpy(coef), rows.shape[1])[:, : 2 * c.n * c.L]
    return z, grads_of


def chain_dense(name: str, dtype=torch.complex128) -> dict:
    """The dense statevector executor (``TorchProgram``) on the same inputs, same keys as ``chain_reference`` /
    ``fused_reference``: complex128 checks the oracle, complex64 is the yardstick of the input conditions."""
    c, i = CHAIN_BY_NAME[name], chain_inputs(name)
    z, grads_of = _chain_dense(c, i, dtype)
    if name.startswith("fused"):
        return _fused_from_z(c, i, z, fused_labels(name), grads_of)
    g = grads_of(i["w"])
    return dict(z=z, grad_s=g, grad=g.reshape(c.K, c.B, -1).sum(1))


CHAIN_KEYS = dict(z="z", grad="grad")
FUSED_KEYS = dict(z="z", dl="dl", grad="fused_grad", loss="loss", lossv="loss")


def within(key: str, got: torch.Tensor, ref: torch.Tensor, frac: float = 1.0):
    """(max error, ok) of ``got`` against the float64 ``ref`` under ``frac`` x the bound named ``key``."""
    d = (got.detach().cpu().double() - ref).abs()
    if key == "loss":
        lim = frac * (TOL["loss_atol"] + TOL["loss_rtol"] * ref.abs())
        return float(d.max()), bool((d <= lim).all())
    return float(d.max()), float(d.max()) <= frac * TOL[key]


# ------------------------------------------------------------------------------------------------ MPO cases
@dataclass(frozen=True)
class MpoCase:
    name: str
    n: int
    build: Callable[[], tuple]     # -> (ops [G, 4], coef [G, 2], n_slots, selector slots)
    readout: tuple
    S: int = 5


_FIXED = ("h", "x", "y", "z", "s", "sdg", "t", "tdg", "sx")
_TWO = {"cx01": ("cx", 0, 1), "cx10": ("cx", 1, 0), "cz01": ("cz", 0, 1), "cz10": ("cz", 1, 0)}


class _B:
    """Circuit builder: every rotation takes the next slot of the vector ``v``."""

    def __init__(self, n: int, n_sel: int = 0):
        self.qc, self.k, self.n_sel = Circuit(n), 0, n_sel
        self.v, self.sel = ParameterVector("v", 128), ParameterVector("sel", max(n_sel, 1))

    def rot(self, kind: str, q: int, scale: float = 1.0):
        getattr(self.qc, kind)(self.v[self.k] * scale, q)
        self.k += 1

    def done(self):
        ops, coef = self.qc.to_program({"v": 0, "sel": self.k})
        return ops, coef, self.k + self.n_sel, tuple(range(self.k, self.k + self.n_sel))


def two_qubits_d16(shift: int):
    """n = 2, the one cut carries CX 0->1, CX 1->0, CZ 0->1, CZ 1->0 (cyclically shifted by ``shift``: each gate type
    and direction lands on every bond bit across the four shifts), with rotations between them."""
    b = _B(2)
    b.rot("ry", 0), b.rot("rx", 1)
    order = list(_TWO)[shift:] + list(_TWO)[:shift]
    for j, g in enumerate(order):
        kind, q0, q1 = _TWO[g]
        getattr(b.qc, kind)(q0, q1)
        b.rot(("rx", "ry", "rz", "p")[j], 0), b.rot(("ry", "p", "rx", "rz")[j], 1)
    b.rot("ry", 0), b.rot("rx", 1)
    return b.done()


def passover4():
    """n = 6: four gates between qubits 1 and 5 pass over qubits 2, 3, 4 (4 pass-through pairs per site); qubit 0 sits
    behind a product cut."""
    b = _B(6)
    for q in range(6):
        b.rot("ry", q)
    b.qc.cx(1, 5), b.qc.cx(5, 1), b.qc.cz(1, 5), b.qc.cz(5, 1)
    for q in range(6):
        b.rot("rx", q), b.rot("p", q), b.rot("rz", q, 0.5)
    return b.done()


def uneven_bonds():
    """n = 6, cut bits [1, 4, 2, 0, 3]: a product cut in the middle and Dl != Dr at most sites."""
    b = _B(6)
    for q in range(6):
        b.rot("ry", q)
    b.qc.cz(1, 0)
    b.rot("rx", 0), b.rot("rz", 1)
    b.qc.cz(3, 1), b.qc.cx(2, 1)
    b.rot("ry", 1), b.rot("rx", 2), b.rot("p", 3)
    b.qc.cx(1, 3), b.qc.cz(1, 2)
    b.qc.cz(5, 4), b.rot("rx", 4), b.qc.cx(5, 4), b.rot("ry", 5), b.qc.cx(4, 5)
    for q in range(6):
        b.rot("rx", q), b.rot("rz", q)
    return b.done()


def idle_qubits():
    """n = 5: no gate at all on qubits 0, 4 and 2; CX / CZ between 1 and 3 pass over the idle qubit 2."""
    b = _B(5)
    b.rot("ry", 1), b.rot("rx", 3)
    b.qc.cx(1, 3)
    b.rot("rz", 1), b.rot("ry", 3)
    b.qc.cz(3, 1)
    b.rot("rx", 1), b.rot("rx", 3), b.rot("p", 3), b.rot("ry", 1)
    return b.done()


def fixed_between_rotations():
    """n = 5: after a CX / CZ end on every qubit, rotation . fixed gate . rotation twice per qubit - every fixed kind,
    the non-diagonal ones between diagonal rotations and vice versa so the order matters - then more entanglers."""
    b = _B(5)
    for q in range(5):
        b.rot("ry", q)
    b.qc.cx(0, 1), b.qc.cx(1, 2), b.qc.cz(2, 3), b.qc.cx(4, 3)
    fixed = _FIXED + ("y",)
    for q in range(5):
        f1, f2 = fixed[2 * q], fixed[2 * q + 1]
        b.rot("rz" if f1 in ("h", "x", "y", "sx") else "rx", q)
        getattr(b.qc, f1)(q)
        b.rot(("p", "ry", "rx", "ry", "p")[q], q)
        getattr(b.qc, f2)(q)
        b.rot(("rx", "ry", "ry", "rx", "rz")[q], q)
    b.qc.cx(2, 0), b.qc.cz(4, 1)
    for q in range(5):
        b.rot(("rx", "ry")[q % 2], q)
    return b.done()


def pauli_selectors():
    """n = 4: a trajectory Pauli (selector from a per-sample slot) between two rotations on every entangled qubit."""
    b = _B(4, n_sel=4)
    for q in range(4):
        b.rot("ry", q)
    b.qc.cx(0, 1), b.qc.cx(1, 2), b.qc.cx(2, 3)
    for q in range(4):
        b.rot(("rx", "rz", "ry", "p")[q], q)
        b.qc.pauli(b.sel[q], q)
        b.rot(("ry", "rx", "rz", "rx")[q], q)
    b.qc.cz(3, 0)
    for q in range(4):
        b.rot("ry", q)
    return b.done()


def maxpg64(extra: int = 0):
    """n = 3: exactly 64 (+ ``extra``) rotations on qubit 1 with one CX on each side in their middle."""
    b = _B(3)
    b.rot("ry", 0), b.rot("rx", 2)
    kinds = [("rx", "ry", "rz", "p")[(j + j // 4) % 4] for j in range(64 + extra)]
    kinds[62], kinds[63] = kinds[63], kinds[62]      # ... rz, ry last: a trailing diagonal gate has no derivative
    for j, kind in enumerate(kinds):
        if j == 20:
            b.qc.cx(0, 1)
        if j == 43:
            b.qc.cx(1, 2)
        b.rot(kind, 1)
    b.rot("rz", 0), b.rot("ry", 2), b.rot("rx", 0)
    return b.done()


def swap3():
    b = _B(3)
    b.rot("ry", 0)
    b.qc.swap(0, 2)
    b.rot("rx", 2)
    return b.done()


def ring4():
    spec = VQCSpec(4, 2, 3, entangler="ring")
    ops, coef = spec.program()
    return ops, coef, spec.n_theta + spec.x_width, ()


def five_on_a_cut():
    b = _B(2)
    b.rot("ry", 0)
    for _ in range(5):
        b.qc.cx(0, 1)
    return b.done()


MPO_CASES = [
    MpoCase("two_qubits_d16", 2, functools.partial(two_qubits_d16, 0), (0,)),                 # qmax = 0, C = 1
    MpoCase("two_qubits_d16_s1", 2, functools.partial(two_qubits_d16, 1), (1, 0)),
    MpoCase("two_qubits_d16_s2", 2, functools.partial(two_qubits_d16, 2), (1,), S=1),
    MpoCase("two_qubits_d16_s3", 2, functools.partial(two_qubits_d16, 3), (0, 1, 1, 0, 0, 0, 1, 1)),
    MpoCase("passover4", 6, passover4, (2, 1)),                                               # stops short of n - 1
    MpoCase("uneven_bonds", 6, uneven_bonds, (5, 0, 3)),
    MpoCase("idle_qubits", 5, idle_qubits, (0, 3, 2, 4)),                                     # <Z> = 1 on idle qubits
    MpoCase("fixed_between_rotations", 5, fixed_between_rotations, (4, 0, 2)),
    MpoCase("pauli_selectors", 4, pauli_selectors, (0, 3)),
    MpoCase("maxpg64", 3, maxpg64, (1, 0, 2)),
    MpoCase("swap3", 3, swap3, (2,), S=1),
    MpoCase("ring4", 4, ring4, (3, 0, 2, 2, 1, 0, 3, 1)),                                     # C = 8, repeats
]
MPO_BY_NAME = {c.name: c for c in MPO_CASES}


def ops_list(ops) -> list:
    return [tuple(int(v) for v in r) for r in np.asarray(ops).tolist()]


@functools.lru_cache(maxsize=None)
def mpo_tables(name: str) -> dict:
    c = MPO_BY_NAME[name]
    return compile_mpo(ops_list(c.build()[0]), c.n)


@functools.lru_cache(maxsize=None)
def mpo_inputs(name: str) -> dict:
    """Seeded float32 inputs: rows [S, n_slots] (rotation slots uniform in [-7, 7]; selector slot j of sample s is
    (s + j) % 4), the gate-angle table ang [S, G] they lower to in float32 - the kernel's input - w [S, C] normal /
    sqrt(C) and mask [G] of the gates whose derivative is reported (slot-carrying rotations)."""
    c = MPO_BY_NAME[name]
    ops, coef, n_slots, sel = c.build()
    rng = np.random.default_rng(_seed(name))
    rows = rng.uniform(-ANGLE, ANGLE, (c.S, n_slots))
    for j, slot in enumerate(sel):
        rows[:, slot] = (np.arange(c.S) + j) % 4
    rows = torch.tensor(rows, dtype=torch.float32)
    ang = gate_angles(torch.from_numpy(ops), torch.from_numpy(coef), rows)
    w = torch.tensor(rng.normal(size=(c.S, len(c.readout))) / np.sqrt(len(c.readout)), dtype=torch.float32)
    mask = torch.tensor([s >= 0 and k in ROTATIONS for k, _, _, s in ops_list(ops)])
    return dict(rows=rows, ang=ang, w=w, mask=mask)


def identity_program(ops, n: int, dtype) -> TorchProgram:
    """The dense executor of the same gates with gate g reading slot g at scale 1: its parameter rows are gate angles."""
    ops = np.array(ops, np.int32)
    ops[:, 3] = np.arange(len(ops))
    coef = np.tile(np.array([[1.0, 0.0]], np.float32), (len(ops), 1))
    return TorchProgram(ops, coef, n, dtype=dtype)


def _mpo_run(name: str, dtype) -> dict:
    c, i = MPO_BY_NAME[name], mpo_inputs(name)
    prog = identity_program(c.build()[0], c.n, dtype)
    ang = i["ang"].to(prog.rdtype)
    psi = prog.run(ang)
    z = prog.expz(psi, list(c.readout))
    dang = prog.adjoint_grads(ang, psi, i["w"].to(prog.rdtype), list(c.readout))
    return dict(psi=psi, z=z, dang=torch.where(i["mask"], dang, torch.zeros_like(dang)))


@functools.lru_cache(maxsize=None)
def mpo_reference(name: str) -> dict:
    """complex128 dense statevector on the float32 gate angles: psi [S, 2^n], z [S, C], dang [S, G] (d/d angle of
    sum_c w_c <Z_c>, masked to the slot-carrying rotations as the kernel wrapper masks its output)."""
    return _mpo_run(name, torch.complex128)


def mpo_dense32(name: str) -> dict:
    return _mpo_run(name, torch.complex64)


def mpo_events(name: str) -> list:
    """Per site, the decoded event list [(type, side, bit, gate kind)] of the compiled tables."""
    tab = mpo_tables(name)
    gk, ev = tab["gkind"].tolist(), tab["events"].tolist()
    return [[(e & 3, (e >> 2) & 1, (e >> 3) & 3, gk[e >> 8]) for e in ev[off:off + cnt]]
            for off, cnt, *_ in tab["sinfo"].tolist()]


# ------------------------------------------------------------------------------------------------ Simulator-level case
def shared_parameter_circuit() -> Circuit:
    """A parameter shared by two gates on different qubits with different coefficients, and a constant-angle rotation
    (slot -1: its derivative is masked out of ``dang``)."""
    v = ParameterVector("v", 4)
    qc = Circuit(4)
    qc.ry(v[0], 0), qc.rx(v[1], 1), qc.ry(v[2], 2), qc.rx(0.9, 3)
    qc.cx(0, 1), qc.cx(3, 2), qc.cz(1, 2)
    qc.rx(v[0] * 0.7 + 0.1, 2), qc.rz(v[1] * -1.3, 0), qc.ry(1.7, 1), qc.p(v[3], 3)
    qc.cx(2, 0)
    qc.ry(v[3] * 0.5, 1), qc.rx(v[2], 0)
    return qc


SIM_READOUT = [0, 2, 3]


@functools.lru_cache(maxsize=None)
def sim_inputs() -> dict:
    rng = np.random.default_rng(11)
    return dict(v=torch.tensor(rng.uniform(-ANGLE, ANGLE, (5, 4)), dtype=torch.float32),
                w=torch.tensor(rng.normal(size=(5, 3)) / np.sqrt(3), dtype=torch.float32))
