"""Quantum natural gradient (QNG): the block-diagonal Fubini-Study metric of the hardware-efficient ansatz and the
damped natural step (Stokes et al. 2020; federated form: Qi 2022).

Every layer of the ansatz (``models/vqc.py circuit()``) is RX(theta_{l,q,0}) RZ(theta_{l,q,1}) on every qubit, then the
entangler.  Gates on different qubits commute, so a layer is an RX sublayer (generators X_q / 2) followed by an RZ
sublayer (generators Z_q / 2): 2L sublayers.  Block b = 2l belongs to the RX sublayer of layer l, its reference state psi
is the state in front of the layer; block b = 2l + 1 to the RZ sublayer, psi the state after the layer's RX gates.  With
generators K_i the block is

    g_ij = Re<psi|K_i K_j|psi> - <psi|K_i|psi><psi|K_j|psi>
         = 1/4 (<P_i P_j> - <P_i><P_j>)   (i != j),     g_ii = 1/4 (1 - <P_i>^2),      P = X (RX block) | Z (RZ block)

and entry (i, j) of block b pairs the flat angles 2 (n l + i) + (b & 1) and 2 (n l + j) + (b & 1).  The metric is per
sample (psi depends on the sample's features); a client's metric is the plain mean over its live samples
(``wmask > 0``), zero for a client without one.  X correlators are the Z correlators of H^n psi.

    theta_block <- theta_block - lr (G_b + damping I)^{-1} grad_block        for every block b
    a, b (readout scale / offset) <- plain gradient step with the same lr

``fubini_study_blocks`` / ``qng_step_ref`` are the float64 reference (the torch backend's implementation and the tests'
oracle); ``MetricProgram`` computes the per-sample correlator records on the GPU (fp32 VALU pass engine for the
cut-point states, ``csrc/qng.hip`` for the correlators); ``csrc/qng.hip qng_step`` is the step on the GPU.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..quantum.circuit import KIND
from .statevec_torch import TorchProgram, _apply_1q, _u1, z_signs

NMAX = 32            # qubits per block the step kernel solves in LDS


def refusal(spec, noise=None, simulator: str = "statevector") -> Optional[str]:
    """Why ``train.optimizer=qng`` does not apply to this model (naming the config key), or None."""
    if simulator != "statevector":
        return (f"train.optimizer=qng needs model.simulator=statevector, got {simulator!r}: the Fubini-Study metric is "
                "a pure-state quantity")
    if noise is not None and (getattr(noise, "gate_noise", False) or spec.noisy):
        return "train.optimizer=qng needs noise.kind=none: the Fubini-Study metric is a pure-state quantity"
    if spec.n_qubits > NMAX:
        return f"train.optimizer=qng solves blocks of model.n_qubits <= {NMAX}, got {spec.n_qubits}"
    if spec.n_qubits < 2:
        return "train.optimizer=qng needs model.n_qubits >= 2"
    return None


def metric_segments(spec) -> dict:
    """Gate indices of the lowered program by segment: ``feature`` (in front of the first layer), and per layer ``rx``
    / ``rz`` (by qubit) and ``ent`` (the entangler behind them)."""
    if spec.noisy:
        raise ValueError("train.optimizer=qng needs noise.kind=none (no trajectory ops in the circuit)")
    ops, _ = spec.program()
    n, L, P = spec.n_qubits, spec.n_layers, spec.n_theta
    seg = {"feature": [], "rx": [[None] * n for _ in range(L)], "rz": [[None] * n for _ in range(L)],
           "ent": [[] for _ in range(L)]}
    layer = -1
    for g, (kind, q0, _q1, slot) in enumerate(ops.tolist()):
        if 0 <= slot < P:
            l, i, r = slot // (2 * n), (slot % (2 * n)) // 2, slot & 1
            if kind != (KIND["rz"] if r else KIND["rx"]) or q0 != i or l < layer:
                raise ValueError("the QNG metric expects the RX / RZ sublayers of models/vqc.py circuit()")
            layer = l
            seg["rz" if r else "rx"][l][i] = g
        elif layer < 0:
            seg["feature"].append(g)
        else:
            seg["ent"][layer].append(g)
    if any(g is None for l in range(L) for g in seg["rx"][l] + seg["rz"][l]):
        raise ValueError("the QNG metric expects one RX and one RZ per qubit and layer")
    return seg


def pair_rows(n: int):
    """(i, j) index vectors of the record's pair entries (i < j, row-major)."""
    iu = torch.triu_indices(n, n, 1)
    return iu[0], iu[1]


def z_correlators(state: torch.Tensor, n: int):
    """<Z_i> [S, n] and <Z_i Z_j> [S, n, n] (float64) of states [S, 2^n]."""
    p = (state.real.double() ** 2 + state.imag.double() ** 2)
    zs = z_signs(n, range(n), state.device, torch.float64)        # [n, N]
    # row-wise sums, not matrix products: a sample's numbers must not depend on the batch it is computed in
    z = (p[:, None, :] * zs[None]).sum(-1)
    zz = torch.stack([((p * zs[i])[:, None, :] * zs[None]).sum(-1) for i in range(n)], 1)
    return z, zz


def blocks_from_correlators(z: torch.Tensor, zz: torch.Tensor) -> torch.Tensor:
    """1/4 (<Z_i Z_j> - <Z_i><Z_j>) with the diagonal 1/4 (1 - <Z_i>^2): z [.., n], zz [.., n, n] -> [.., n, n]."""
    n = z.shape[-1]
    eye = torch.eye(n, dtype=torch.bool, device=z.device)
    zz = torch.where(eye, torch.ones_like(zz), zz)
    return 0.25 * (zz - z.unsqueeze(-1) * z.unsqueeze(-2))


def records_to_blocks(rec: torch.Tensor, n: int) -> torch.Tensor:
    """Per-sample records [.., n (n + 1) / 2] = [<Z_i> | <Z_i Z_j> (i < j)] -> per-sample blocks [.., n, n]."""
    i, j = pair_rows(n)
    z = rec[..., :n]
    zz = torch.zeros(*rec.shape[:-1], n, n, dtype=rec.dtype, device=rec.device)
    zz[..., i, j] = rec[..., n:]
    zz[..., j, i] = rec[..., n:]
    return blocks_from_correlators(z, zz)


def client_blocks(per_sample: torch.Tensor, wmask: torch.Tensor) -> torch.Tensor:
    """Per-sample blocks [K, B, ...] -> the clients' blocks [K, ...]: the mean over live samples, zero without one."""
    live = (wmask > 0).to(per_sample.dtype)
    shape = live.shape + (1,) * (per_sample.dim() - 2)
    cnt = live.sum(1).clamp(min=1.0)
    return (per_sample * live.reshape(shape)).sum(1) / cnt.reshape((-1,) + (1,) * (per_sample.dim() - 2))


@torch.no_grad()
def fubini_study_blocks(spec, xang: torch.Tensor, theta: torch.Tensor, init: Optional[torch.Tensor] = None):
    """Per-sample metric blocks [K, B, 2L, n, n] in float64.  ``xang`` [K, B, x_width] encoded features, ``theta``
    [K, >= n_theta] per-client angles, ``init`` (amplitude encoding) raw amplitudes [K, B, <= 2^n] or complex states.
    One walk of the program (sublayer by sublayer: gates on different qubits commute), the correlators read at the 2L
    cut points."""
    why = refusal(spec)
    if why:
        raise ValueError(why)
    seg = metric_segments(spec)
    ops, coef = spec.program()
    n, L = spec.n_qubits, spec.n_layers
    K, B, _ = xang.shape
    dev = xang.device
    prog = TorchProgram(ops, coef, n, dev, torch.complex128)
    th = theta[:, None, :spec.n_theta].expand(K, B, spec.n_theta).double()
    rows = torch.cat([th, xang.double()], -1).reshape(K * B, -1)
    ang = prog.angles(rows)
    if spec.amplitude:
        if init is None:
            raise ValueError("amplitude-encoded VQC needs init [K, B, <=2^n]")
        st = (init if init.is_complex() else spec.initial_states(init.double())).reshape(K * B, -1).to(prog.dtype)
        st = st / st.abs().pow(2).sum(-1, keepdim=True).sqrt()
    else:
        st = prog.initial_state(K * B)
    hadamard = _u1(KIND["h"], torch.zeros(K * B, dtype=torch.float64, device=dev), prog.dtype)

    def run(state, gates):
        for g in gates:
            state = prog.apply_gate(state, g, ang[:, g])
        return state

    st = run(st, seg["feature"])
    out = torch.zeros(K * B, 2 * L, n, n, dtype=torch.float64, device=dev)
    for l in range(L):
        hs = st
        for q in range(n):
            hs = _apply_1q(hs, q, hadamard)
        out[:, 2 * l] = blocks_from_correlators(*z_correlators(hs, n))
        st = run(st, seg["rx"][l])
        out[:, 2 * l + 1] = blocks_from_correlators(*z_correlators(st, n))
        st = run(st, seg["rz"][l] + seg["ent"][l])
    return out.reshape(K, B, 2 * L, n, n)


def block_slots(spec, device=None) -> torch.Tensor:
    """[2L, n] flat angle index of entry i of block b: 2 (n l + i) + (b & 1)."""
    n, L = spec.n_qubits, spec.n_layers
    b = torch.arange(2 * L, device=device)[:, None]
    i = torch.arange(n, device=device)[None, :]
    return 2 * (n * (b // 2) + i) + (b & 1)


@torch.no_grad()
def qng_step_ref(params: torch.Tensor, grad: torch.Tensor, G: torch.Tensor, active: Optional[torch.Tensor], lr: float,
                 damping: float, spec) -> torch.Tensor:
    """The damped natural step in float64, in place on the active rows of ``params`` [K, P] (inactive rows keep their
    bits).  ``G`` [K, 2L, n, n] the clients' metric blocks; the readout entries a / b take the plain step."""
    if not damping > 0:
        raise ValueError(f"train.qng_damping must be > 0, got {damping}")
    K, P = params.shape
    n, L = spec.n_qubits, spec.n_layers
    if tuple(G.shape) != (K, 2 * L, n, n):
        raise ValueError(f"metric blocks must be [K, 2L, n, n] = {(K, 2 * L, n, n)}, got {tuple(G.shape)}")
    slots = block_slots(spec, params.device)
    g64 = grad.double()
    nat = g64.clone()                                            # a / b: identity metric
    A = G.double() + damping * torch.eye(n, dtype=torch.float64, device=G.device)
    nat[:, slots.reshape(-1)] = torch.linalg.solve(A, g64[:, slots].unsqueeze(-1)).squeeze(-1).reshape(K, -1)
    new = (params.double() - lr * nat).to(params.dtype)
    on = torch.ones(K, dtype=torch.bool, device=params.device) if active is None else active > 0
    params.copy_(torch.where(on[:, None], new, params))
    return params


class MetricProgram:
    """The per-sample correlator records of the 2L cut points on the GPU.

    The circuit is lowered into segments - the feature map, each RX sublayer, each RZ sublayer + entangler, one H^n -
    and ONE state buffer advances through them with the planner's load-from-state mode (no prefix is run twice); at an
    RX cut H^n psi goes into a second buffer.  The segments run on the fp32 VALU pass engine's ahead-of-time pass
    kernel (``csrc/statevec.hip``), whichever engine produces the gradient (the MFMA engine keeps fp16 frame-addressed
    states): a segment is one memory-bound sweep of n one-qubit gates, and its forward store plan is the only plan
    built.  The correlators of a buffer come from ``csrc/qng.hip`` in one more sweep.  Samples run in chunks of whole
    states that fit the budget; a sample's record does not depend on its chunk."""

    def __init__(self, spec, device, kmax: Optional[int] = None):
        from .plan_tools import FIN_STORE
        from .statevec_hip import KMAX, MODE_FWD_LOAD, _Plan, choose_R
        why = refusal(spec)
        if why:
            raise ValueError(why)
        if spec.n_qubits > 30:
            raise ValueError("the statevector pass planner holds model.n_qubits <= 30")
        self.spec = spec
        self.n, self.L = spec.n_qubits, spec.n_layers
        self.device = torch.device(device)
        ops, coef = spec.program()
        seg = metric_segments(spec)
        R = choose_R(self.n)
        kmax = KMAX if kmax is None else kmax

        def plan(o, c):
            return _Plan(torch.as_tensor(o, dtype=torch.int32).reshape(-1, 4),
                         torch.as_tensor(c, dtype=torch.float32).reshape(-1, 2), self.n, R, kmax, spec.readout,
                         spec.n_theta, MODE_FWD_LOAD, FIN_STORE, self.device, False)

        def sub(gates):
            return plan(ops[gates], coef[gates]) if gates else None

        self.feature = sub(seg["feature"])
        self.rx = [sub(seg["rx"][l]) for l in range(self.L)]
        self.rz_ent = [sub(seg["rz"][l] + seg["ent"][l]) for l in range(self.L)]
        self.hadamard = plan([[KIND["h"], q, -1, -1] for q in range(self.n)], [[0.0, 0.0]] * self.n)
        self.rec_width = self.n * (self.n + 1) // 2
        self._ws = {}

    def _buf(self, name: str, numel: int, dtype) -> torch.Tensor:
        t = self._ws.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.empty(numel, dtype=dtype, device=self.device)
            self._ws[name] = t
        return t[:numel]

    def _run(self, plan, psi, rows, x, S: int) -> None:
        from ._ext import ext
        if plan is None:
            return
        for off, k, ngrad, nops in plan.passes:
            ext().pass_launch(plan.R, False, plan.blob, off, k, self.n, nops, plan.info["G"], psi, None, rows, 1, x,
                              None, None, None, S, ngrad)

    def state_bytes(self) -> int:
        """Bytes of the two state buffers of one sample."""
        return 2 * 8 * (1 << self.n)

    @torch.no_grad()
    def records(self, xang: torch.Tensor, theta: torch.Tensor, init: Optional[torch.Tensor], budget: int):
        """rec [K * B, 2L, n (n + 1) / 2] float64: every sample's [<P_i> | <P_i P_j> (i < j)] at every cut (P = X at the
        RX cuts, Z at the RZ cuts)."""
        from ._ext import ext
        C = ext()
        spec, n, L = self.spec, self.n, self.L
        K, B, F = xang.shape
        S, N = K * B, 1 << n
        per = int(budget) // self.state_bytes()
        if per < 1:
            raise ValueError(f"train.optimizer=qng needs two states of one sample in the state budget: "
                             f"model.n_qubits={n} needs {self.state_bytes()} bytes, the budget is {int(budget)}")
        per = min(per, S)
        # one parameter row per sample, so that a chunk is any run of samples
        rows = theta[:, None, :].expand(K, B, theta.shape[-1]).reshape(S, -1).float().contiguous()
        x = xang.reshape(S, F).float().contiguous()
        if spec.amplitude:
            if init is None:
                raise ValueError("amplitude-encoded VQC needs init [K, B, <=2^n]")
            init = init.reshape(S, -1)
        rec = torch.empty(S, 2 * L, self.rec_width, dtype=torch.float64, device=self.device)
        psi = self._buf("psi", per * N, torch.complex64)
        phi = self._buf("phi", per * N, torch.complex64)
        trec = self._buf("trec", per * int(C.qng_tiles(n)) * int(C.qng_tile_rec()), torch.float32)
        for r0 in range(0, S, per):
            Sc = min(per, S - r0)
            ps, ph = psi[:Sc * N], phi[:Sc * N]
            rw, xs = rows[r0:r0 + Sc], x[r0:r0 + Sc]
            if spec.amplitude:
                self._state_in(ps, init[r0:r0 + Sc])
            else:
                ps.zero_()
                ps.view(Sc, N)[:, 0] = 1.0
            self._run(self.feature, ps, rw, xs, Sc)
            for l in range(L):
                ph.copy_(ps)
                self._run(self.hadamard, ph, rw, xs, Sc)
                C.qng_corr(ph.view(Sc, N), n, trec, rec, r0, 2 * l)
                self._run(self.rx[l], ps, rw, xs, Sc)
                C.qng_corr(ps.view(Sc, N), n, trec, rec, r0, 2 * l + 1)
                if l + 1 < L:
                    self._run(self.rz_ent[l], ps, rw, xs, Sc)
        return rec

    def _state_in(self, psi: torch.Tensor, init: torch.Tensor) -> None:
        """Initial states of a chunk: complex ``init`` as given, real ``init`` = raw amplitudes encoded on the device
        (float64 normalisation, as ``HipProgram._state_in``)."""
        from ._ext import ext
        if init.is_complex():
            psi.view(init.shape[0], -1).copy_(init.to(torch.complex64))
            return
        xr = init.float().contiguous()
        part = self._buf("amp_part", xr.shape[0] * ext().amp_scratch(xr.shape[1]), torch.float64)
        ext().amp_init(xr, self.n, part, psi)
