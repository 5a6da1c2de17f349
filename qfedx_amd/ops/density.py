"""Exact density-matrix simulator for small noisy VQCs (ROADMAP.md:64-73).

The statevector engines realise gate noise as Pauli-channel trajectories, which is exact for depolarizing noise
but only the Pauli twirl of amplitude damping.  ``model.simulator=density`` (auto-selected for
``noise.kind=amplitude``) runs every sample's circuit as a density matrix instead, with the gate-noise channel as
its exact Kraus operators after every gate:

  * HIP: ``csrc/density.hip`` - one workgroup per circuit instance, rho in LDS up to 6 qubits, an L2-resident
    global slab up to 10; a one-qubit gate and its channel are ONE 4 x 4 superoperator pass
  * torch: the same superoperator passes on a [S, 2^n, 2^n] complex128 tensor (CPU path and test oracle)

Readout confusion and shots apply to the exact <Z> as on the other engines.  Gradients: a reverse sweep
(``DensityProgram.vjp``; ``train.grad_method=adjoint | autograd`` with exact readout), parameter shift (valid for the
exp(-i theta P / 2) rotations with parameter-independent channels in between; the route under ``noise.shots`` > 0) or
SPSA.

The reverse sweep.  <O> = sum_c w_c <Z_c> = <Lambda_G, rho_G> with Lambda_G = diag(sum_c w_c (1 - 2 r_c)) and
<A, B> = sum_i conj(A_i) B_i.  Every gate is linear on rho, so Lambda pulls back gate by gate, Lambda_{g-1} =
T_g^dagger Lambda_g (two-qubit gates: S^dagger on both qubits, then the self-inverse permutation / sign), and a
rotation exp(-i ang P / 2) has dT/d(ang) = T Gen with Gen rho = -(i / 2) [P, rho]:
    d<O>/d(ang_g) = Re <T_g^dagger Lambda_g, Gen rho_{g-1}>.
The channels cannot be run backwards, so the forward sweep keeps rho_{g-1} of every differentiated gate: the tape,
``tape_bytes`` = J 4^n 8 bytes per sample on the GPU (J gates on slots below ``n_grad``; 4q x 2L: 32 KB, 8q x 3L:
24 MB, 10q x 1L: 160 MB).  ``vjp`` runs the samples in chunks whose tape fits a byte budget (``QFEDX_DM_TAPE_MB``).
  * HIP: ``csrc/density_adj.hip`` - one workgroup per sample in both sweeps, one pass per gate, fixed-order reductions
  * torch: ``_vjp_torch``, the same sweep in float64 (CPU path)
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from ..quantum.circuit import KIND, gate_matrix

MAX_QUBITS = 10
_INV = {v: k for k, v in KIND.items()}
_PARAM = {"rx", "ry", "rz", "p"}
_TWO = {"cx", "cz", "swap"}

_I = np.eye(2, dtype=complex)
_X = np.array([[0, 1], [1, 0]], complex)
_Y = np.array([[0, -1j], [1j, 0]])
_Z = np.diag([1.0, -1.0]).astype(complex)


def kraus_ops(kind: str, p: float = 0.0, gamma: float = 0.0) -> list[np.ndarray]:
    """Kraus operators of the per-gate channel: ``depolarizing`` (p: X, Y, Z with p / 3 each), ``amplitude``
    (exact amplitude damping: K0 = diag(1, sqrt(1 - gamma)), K1 = sqrt(gamma) |0><1|), ``amplitude_twirl`` (its
    Pauli twirl, what the statevector trajectories realise)."""
    kind = (kind or "none").lower()
    if kind in ("none", "ideal", ""):
        return [_I]
    if kind in ("depolarizing", "depolarising", "dep"):
        return [math.sqrt(1 - p) * _I, math.sqrt(p / 3) * _X, math.sqrt(p / 3) * _Y, math.sqrt(p / 3) * _Z]
    if kind in ("amplitude", "amplitude_damping", "amp"):
        return [np.diag([1.0, math.sqrt(max(0.0, 1.0 - gamma))]).astype(complex),
                np.array([[0.0, math.sqrt(gamma)], [0.0, 0.0]], complex)]
    if kind in ("amplitude_twirl", "amp_twirl"):
        from ..quantum.noise import pauli_probs
        px, py, pz = pauli_probs(kind, p, gamma)
        return [math.sqrt(max(0.0, 1 - px - py - pz)) * _I, math.sqrt(px) * _X, math.sqrt(py) * _Y,
                math.sqrt(pz) * _Z]
    raise ValueError(f"unknown noise kind '{kind}'")


def superop(kraus: list[np.ndarray]) -> np.ndarray:
    """4 x 4 S[(a, b)][(a', b')] = sum_i K_i[a][a'] conj(K_i[b][b']) over quad index a + 2 b (a: row bit,
    b: column bit of the qubit)."""
    S = np.zeros((4, 4), complex)
    for K in kraus:
        for r in range(4):
            for c in range(4):
                S[r, c] += K[r & 1, c & 1] * np.conj(K[r >> 1, c >> 1])
    return S


def generator_superop(pauli: np.ndarray) -> np.ndarray:
    """4 x 4 Gen = -(i / 2) [P, .] over quad index a + 2 b: the derivative of the superoperator of
    exp(-i ang P / 2) with respect to ang is T Gen = Gen T."""
    G = np.zeros((4, 4), complex)
    for r in range(4):
        for c in range(4):
            a, b, a2, b2 = r & 1, r >> 1, c & 1, c >> 1
            G[r, c] = -0.5j * (pauli[a, a2] * (b == b2) - (a == a2) * pauli[b2, b])
    return G


_GEN = {"rx": generator_superop(_X), "ry": generator_superop(_Y), "rz": generator_superop(_Z)}
_GEN["p"] = _GEN["rz"]                 # p(phi) = e^{i phi / 2} rz(phi): the phase drops out of U rho U^dagger


def lower(ops: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """Program (ops [G, 4] kind/q0/q1/slot, coef [G, 2] scale/offset) -> the kernel's gate records as int32 words
    [G, 14]: kind, q0, q1, slot, scale, off (float bits), fixed 2 x 2 matrix (re, im) x 4 (float bits)."""
    rec = np.zeros((len(ops), 14), dtype=np.int32)
    fl = rec.view(np.float32)
    for g, ((kind, q0, q1, slot), (sc, off)) in enumerate(zip(np.asarray(ops).tolist(), np.asarray(coef).tolist())):
        name = _INV[int(kind)]
        if name in ("pauli", "unitary", "initialize"):
            raise ValueError(f"the density-matrix simulator does not run '{name}' ops")
        rec[g, :4] = (int(kind), int(q0), int(q1), int(slot))
        fl[g, 4], fl[g, 5] = float(sc), float(off)
        if name not in _PARAM and name not in _TWO:
            m = gate_matrix(name)
            fl[g, 6:14] = np.stack([m.real, m.imag], -1).reshape(-1).astype(np.float32)
    return rec


class DensityProgram:
    """Batched exact density-matrix evaluation of one lowered program: ``expz(rows)`` -> <Z_c> [S, C];
    ``vjp(rows, w, n_grad)`` -> <Z_c> and the per-gate angle gradients of sum_c w_c <Z_c>."""

    def __init__(self, ops, coef, n_qubits: int, readout, device, kraus: list[np.ndarray] | None = None):
        if n_qubits > MAX_QUBITS:
            raise ValueError(f"density-matrix simulation is for <= {MAX_QUBITS} qubits (got {n_qubits}); use the "
                             "statevector engine with noise.kind=amplitude_twirl / depolarizing trajectories")
        self.n = n_qubits
        self.ops = np.asarray(ops)
        self.coef = np.asarray(coef)
        self.readout = [int(c) for c in readout]
        self.device = torch.device(device)
        self.S = superop(kraus) if kraus is not None and len(kraus) > 1 else None
        self.chi_max = 1
        if self.device.type == "cuda":
            from ._ext import ext
            E = ext()
            if E.dm_gate_bytes() != 56:
                raise RuntimeError("density gate record layout mismatch")
            self._gates = torch.from_numpy(lower(self.ops, self.coef).reshape(-1)).to(self.device)
            self._ro = torch.tensor(self.readout, dtype=torch.int32, device=self.device)
            self._sup = (torch.from_numpy(np.stack([self.S.real, self.S.imag], -1).reshape(-1).astype(np.float32))
                         .to(self.device) if self.S is not None else torch.zeros(0, device=self.device))
            self._lds = E.dm_lds_qubits()

    def state_bytes(self) -> int:
        return (1 << (2 * self.n)) * 8

    @torch.no_grad()
    def expz(self, rows: torch.Tensor) -> torch.Tensor:
        rows = rows.float().contiguous()
        S = rows.shape[0]
        C = len(self.readout)
        if S == 0:
            return torch.zeros(0, C, device=rows.device)
        if self.device.type == "cuda":
            from ._ext import ext
            out = torch.empty(S, C, dtype=torch.float32, device=self.device)
            scratch = (torch.empty(S << (2 * self.n), dtype=torch.complex64, device=self.device)
                       if self.n > self._lds else torch.zeros(0, dtype=torch.complex64, device=self.device))
            ext().dm_run(self._gates, len(self.ops), self.n, rows, self._ro, self._sup, scratch, out)
            return out
        return self._expz_torch(rows.double()).float()

    # ------------------------------------------------------------------ reverse sweep
    def taped_gates(self, n_grad: int) -> list[int]:
        """The gates the reverse sweep differentiates: parametrised one-qubit gates on slots [0, n_grad)."""
        return [g for g, (kind, _, _, slot) in enumerate(self.ops.tolist())
                if _INV[int(kind)] in _PARAM and 0 <= slot < n_grad]

    def tape_bytes(self, n_grad: int) -> int:
        """Bytes of tape one sample needs: rho in front of every differentiated gate (complex64 on the GPU,
        complex128 on the torch path)."""
        return len(self.taped_gates(n_grad)) * self.state_bytes() * (1 if self.device.type == "cuda" else 2)

    @torch.no_grad()
    def vjp(self, rows: torch.Tensor, w, n_grad: int, budget: int | None = None):
        """One forward sweep with tape and one backward sweep per sample -> (<Z_c> [S, C], gg [S, G]) with
        gg[s, g] = d(sum_c w[s, c] <Z_c>[s]) / d(angle of gate g), 0 for gates that are not differentiated.

        ``w`` is [S, C], or a callable ``w(expz [m, C], lo, hi) -> [m, C]`` for weights that depend on the rows' own
        <Z> (a loss on the readout): it is called once per chunk of rows lo..hi.  The samples run in chunks whose tape
        fits ``budget`` bytes (``QFEDX_DM_TAPE_MB`` overrides it; None: one chunk); a row's result does not depend on
        the chunking.  float32 on the GPU; on the CPU <Z> is float32 (as ``expz``) and gg float64."""
        S, C, G = rows.shape[0], len(self.readout), len(self.ops)
        cuda = self.device.type == "cuda"
        if os.environ.get("QFEDX_DM_TAPE_MB"):
            budget = int(float(os.environ["QFEDX_DM_TAPE_MB"]) * (1 << 20))
        per = self.tape_bytes(n_grad)
        chunk = max(S, 1)
        if budget is not None and per > 0:
            chunk = min(chunk, int(budget) // per)
            if chunk < 1:
                raise ValueError(f"the reverse sweep's tape needs {per} bytes per sample ({len(self.taped_gates(n_grad))}"
                                 f" gates x 4^{self.n} entries), over the budget of {int(budget)} bytes; raise "
                                 "QFEDX_DM_TAPE_MB or use train.grad_method=param_shift")
        rows = rows.float().contiguous() if cuda else rows.double()
        sweep = self._vjp_hip if cuda else self._vjp_torch
        if 0 < S <= chunk:
            return sweep(rows, w, n_grad, 0, S)
        expz = torch.zeros(S, C, dtype=torch.float32, device=rows.device)
        gg = torch.zeros(S, G, dtype=torch.float32 if cuda else torch.float64, device=rows.device)
        for lo in range(0, S, chunk):
            hi = min(S, lo + chunk)
            z, g = sweep(rows[lo:hi], w, n_grad, lo, hi)
            expz[lo:hi] = z
            gg[lo:hi] = g
        return expz, gg

    @staticmethod
    def _weights(w, z: torch.Tensor, lo: int, hi: int) -> torch.Tensor:
        w = w(z, lo, hi) if callable(w) else w[lo:hi]
        if w.shape != z.shape:
            raise ValueError(f"vjp: w must be [S, C] = {tuple(z.shape)} per chunk, got {tuple(w.shape)}")
        return w

    def _vjp_hip(self, rows: torch.Tensor, w, n_grad: int, lo: int, hi: int):
        from ._ext import ext
        E = ext()
        S, C, G, N = rows.shape[0], len(self.readout), len(self.ops), 1 << (2 * self.n)
        J = len(self.taped_gates(n_grad))
        dev = self.device
        z = torch.empty(S, C, dtype=torch.float32, device=dev)
        gg = torch.empty(S, G, dtype=torch.float32, device=dev)
        tape = torch.empty(S * J * N, dtype=torch.complex64, device=dev)
        # rho (forward) and Lambda (backward) share one slab past the LDS sizes
        slab = torch.empty(S * N if self.n > self._lds else 0, dtype=torch.complex64, device=dev)
        E.dm_forward_tape(self._gates, G, self.n, rows, self._ro, self._sup, slab, n_grad, J, tape, z)
        wt = self._weights(w, z, lo, hi).to(dev).float().contiguous()
        E.dm_adjoint(self._gates, G, self.n, rows, self._ro, self._sup, n_grad, J, tape, slab, wt, gg)
        return z, gg

    # ------------------------------------------------------------------ torch path (CPU / oracle)
    def _apply_quad(self, rho: torch.Tensor, q: int, T: torch.Tensor) -> torch.Tensor:
        """rho [S, 2^n (rows), 2^n (cols)]; T [S or 1, 4, 4] on (row bit q, col bit q)."""
        S, D = rho.shape[0], 1 << self.n
        hi = D >> (q + 1)
        lo = 1 << q
        r = rho.reshape(S, hi, 2, lo, hi, 2, lo)                     # [S, rh, a, rl, ch, b, cl]
        v = r.permute(0, 1, 3, 4, 6, 5, 2).reshape(S, -1, 4)        # quad index a + 2 b -> (b, a) order
        v = torch.einsum("sij,smj->smi", T.expand(S, 4, 4), v)
        v = v.reshape(S, hi, lo, hi, lo, 2, 2).permute(0, 1, 6, 2, 3, 5, 4)
        return v.reshape(S, D, D)

    # The reverse sweep keeps its own gate helpers: _expz_torch below is the oracle its tests shift through
    # (tests/density_adjoint_cases.py) and shares only _apply_quad with it.
    def _two_qubit(self, rho: torch.Tensor, name: str, q0: int, q1: int) -> torch.Tensor:
        """cx / cz / swap on rows and columns (each is its own inverse, so the pull-back uses it as it stands)."""
        idx = torch.arange(1 << self.n, device=rho.device)
        if name == "cz":
            z = 1 - 2 * (((idx >> q0) & (idx >> q1)) & 1)
            return rho * (z[:, None] * z[None, :]).to(rho.dtype)
        if name == "cx":
            perm = torch.where(((idx >> q0) & 1).bool(), idx ^ (1 << q1), idx)
        else:
            b0, b1 = (idx >> q0) & 1, (idx >> q1) & 1
            perm = torch.where(b0 != b1, idx ^ ((1 << q0) | (1 << q1)), idx)
        return rho[:, perm][:, :, perm]

    def _gate_superop(self, name: str, rows: torch.Tensor, slot: int, sc: float, off: float) -> torch.Tensor:
        """T = S (U (x) U*) [S, 4, 4] of a one-qubit gate over quad index a + 2 b."""
        S = rows.shape[0]
        if name in _PARAM:
            ang = (sc * (rows[:, slot] if slot >= 0 else torch.zeros_like(rows[:, 0])) + off).cpu().numpy()
            U = torch.from_numpy(np.stack([gate_matrix(name, float(a)) for a in ang]))
        else:
            U = torch.from_numpy(gate_matrix(name))[None].expand(S, 2, 2)
        T = torch.einsum("sac,sbd->sbadc", U, U.conj()).reshape(S, 4, 4)    # row b * 2 + a, col b' * 2 + a'
        if self.S is not None:
            T = torch.einsum("ij,sjk->sik", torch.from_numpy(self.S), T)
        return T.to(rows.device)

    def _vjp_torch(self, rows: torch.Tensor, w, n_grad: int, lo: int = 0, hi: int | None = None):
        """The reverse sweep in float64 -> (<Z_c> [S, C] float32, gg [S, G] float64)."""
        S, D, G = rows.shape[0], 1 << self.n, len(self.ops)
        hi = lo + S if hi is None else hi
        rows = rows.double()
        prog = list(zip(self.ops.tolist(), self.coef.tolist()))
        taped = set(self.taped_gates(n_grad))
        Sn = torch.from_numpy(self.S)[None] if self.S is not None else None
        rho = torch.zeros(S, D, D, dtype=torch.complex128, device=rows.device)
        rho[:, 0, 0] = 1.0
        tape, Ts = {}, {}
        for g, ((kind, q0, q1, slot), (sc, off)) in enumerate(prog):
            name = _INV[int(kind)]
            if name in _TWO:
                rho = self._two_qubit(rho, name, q0, q1)
                if Sn is not None:
                    rho = self._apply_quad(self._apply_quad(rho, q0, Sn), q1, Sn)
                continue
            if g in taped:
                tape[g] = rho
            Ts[g] = self._gate_superop(name, rows, slot, sc, off)
            rho = self._apply_quad(rho, q0, Ts[g])
        idx = torch.arange(D, device=rows.device)
        sign = torch.stack([1 - 2 * ((idx >> c) & 1) for c in self.readout]).double()        # [C, D]
        expz = (torch.diagonal(rho, dim1=1, dim2=2).real @ sign.T).float()
        wt = self._weights(w, expz, lo, hi).to(rows.device).double()
        lam = torch.diag_embed((wt @ sign).to(torch.complex128))                            # Lambda_G
        gg = torch.zeros(S, G, dtype=torch.float64, device=rows.device)
        Sd = Sn.conj().transpose(-1, -2) if Sn is not None else None
        for g in range(G - 1, -1, -1):
            (kind, q0, q1, slot), _ = prog[g]
            name = _INV[int(kind)]
            if name in _TWO:
                if Sd is not None:
                    lam = self._apply_quad(self._apply_quad(lam, q1, Sd), q0, Sd)
                lam = self._two_qubit(lam, name, q0, q1)
                continue
            lam = self._apply_quad(lam, q0, Ts[g].conj().transpose(-1, -2))
            if g in taped:
                gen = torch.from_numpy(_GEN[name])[None].to(rows.device)
                gg[:, g] = (lam.conj() * self._apply_quad(tape[g], q0, gen)).sum((1, 2)).real
        return expz, gg

    def _expz_torch(self, rows: torch.Tensor) -> torch.Tensor:
        S, D = rows.shape[0], 1 << self.n
        rho = torch.zeros(S, D, D, dtype=torch.complex128, device=rows.device)
        rho[:, 0, 0] = 1.0
        Sn = torch.from_numpy(self.S) if self.S is not None else None
        idx = torch.arange(D, device=rows.device)
        for (kind, q0, q1, slot), (sc, off) in zip(self.ops.tolist(), self.coef.tolist()):
            name = _INV[int(kind)]
            if name in _TWO:
                if name == "cz":
                    z = 1 - 2 * (((idx >> q0) & (idx >> q1)) & 1)
                    zz = (z[:, None] * z[None, :]).to(rho.dtype)
                    rho = rho * zz
                else:
                    if name == "cx":
                        perm = torch.where(((idx >> q0) & 1).bool(), idx ^ (1 << q1), idx)
                    else:
                        b0, b1 = (idx >> q0) & 1, (idx >> q1) & 1
                        perm = torch.where(b0 != b1, idx ^ ((1 << q0) | (1 << q1)), idx)
                    rho = rho[:, perm][:, :, perm]
                if Sn is not None:
                    rho = self._apply_quad(rho, q0, Sn[None])
                    rho = self._apply_quad(rho, q1, Sn[None])
                continue
            if name in _PARAM:
                ang = (sc * (rows[:, slot] if slot >= 0 else torch.zeros_like(rows[:, 0])) + off).cpu().numpy()
                U = torch.from_numpy(np.stack([gate_matrix(name, float(a)) for a in ang]))
            else:
                U = torch.from_numpy(gate_matrix(name))[None].expand(S, 2, 2)
            UU = torch.einsum("sac,sbd->sabcd", U, U.conj())        # [(a, b), (a', b')] with a + 2 b order below
            T = UU.permute(0, 2, 1, 4, 3).reshape(S, 4, 4)          # row index b * 2 + a, col b' * 2 + a'
            if Sn is not None:
                T = torch.einsum("ij,sjk->sik", Sn, T)
            rho = self._apply_quad(rho, q0, T.to(rho.device))
        diag = torch.diagonal(rho, dim1=1, dim2=2).real
        return torch.stack([(diag * (1 - 2 * ((idx >> c) & 1))).sum(-1) for c in self.readout], -1)
