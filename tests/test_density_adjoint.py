"""Reverse-mode gradients of the density-matrix simulator on the CPU: ops/density.py ``vjp`` / ``_vjp_torch`` against
the float64 shift-rule oracle of tests/density_adjoint_cases.py, and the engine's adjoint route on this simulator."""
import numpy as np
import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops.density import DensityProgram
from qfedx_amd.ops.engine import VQCEngine
from qfedx_amd.quantum.noise import NoiseModel
from tests.density_adjoint_cases import hand_case, oracle, vqc_case


def _readout(n, C):
    return [n - 1] if C == 1 else [0, n - 1, 1 % n]


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("entangler", ["chain", "ring"])
@pytest.mark.parametrize("kind,p,gamma", [("amplitude", 0.0, 0.25), ("depolarizing", 0.1, 0.0), ("none", 0.0, 0.0)])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_vjp_torch_matches_shift_oracle(n, kind, p, gamma, entangler, C):
    prog, rows, w, n_grad = vqc_case(n, 2, kind, p, gamma, entangler, _readout(n, C))
    z, gg = prog._vjp_torch(rows.double(), w, n_grad)
    zr, gr = oracle(prog, rows, w, n_grad)
    assert gg.dtype == torch.float64 and gr.abs().max() > 1e-3
    assert (gg - gr).abs().max() < 1e-9
    assert (z.double() - zr).abs().max() < 1e-6          # <Z> is handed out in float32, as expz() does


def test_hand_built_program_matches_shift_oracle():
    prog, rows, w, n_grad = hand_case()
    z, gg = prog._vjp_torch(rows.double(), w, n_grad)
    zr, gr = oracle(prog, rows, w, n_grad)
    assert (gg - gr).abs().max() < 1e-9
    taped = prog.taped_gates(n_grad)
    assert taped == [1, 3, 5, 6]                          # rx(t0), ry(2 t1 + .3), p(t0), rz(t2); not rx(t3)
    rest = [g for g in range(len(prog.ops)) if g not in taped]
    assert torch.equal(gg[:, rest], torch.zeros(3, len(rest), dtype=torch.float64))
    # (p on qubit 2 and rz on qubit 1 sit in front of a cx control / nothing and a Z readout: their gradients vanish)
    assert gr[:, [1, 3]].abs().min() > 1e-3 and gr[:, [5, 6]].abs().max() < 1e-12
    # central differences on the slots agree too (t0 drives two gates; t1 through its scale 2)
    from qfedx_amd.ops.statevec_torch import slot_grads
    gs = slot_grads(gg, torch.from_numpy(prog.ops), torch.from_numpy(prog.coef), 4)
    h = 1e-5
    for j in range(4):
        d = torch.zeros(4, dtype=torch.float64)
        d[j] = h
        fd = ((prog._expz_torch(rows.double() + d) - prog._expz_torch(rows.double() - d)) * w.double()).sum(-1) / (2 * h)
        assert (gs[:, j] - (fd if j < 3 else 0.0)).abs().max() < 1e-8


def _engine_setup(noise, n=3, L=2, K=2, B=3):
    spec = VQCSpec(n, L, 3, readout_scale=2.0, init_std=1.0)
    g = torch.Generator().manual_seed(1)
    x = spec.encode_features(torch.rand(K, B, n, generator=g))
    y = torch.randint(0, 3, (K, B), generator=g)
    w = torch.full((K, B), 1.0 / B)
    params = torch.stack([spec.init_params(k) for k in range(K)])
    return spec, VQCEngine(spec, "cpu", "density", noise=noise), x, y, w, params


class _Count:
    """Counts the circuit evolutions (rows) that pass through DensityProgram.expz / vjp."""

    def __init__(self, monkeypatch):
        self.expz = self.vjp = 0
        expz0, vjp0 = DensityProgram.expz, DensityProgram.vjp

        def expz(prog, rows):
            self.expz += rows.shape[0]
            return expz0(prog, rows)

        def vjp(prog, rows, *a, **k):
            self.vjp += rows.shape[0]
            return vjp0(prog, rows, *a, **k)

        monkeypatch.setattr(DensityProgram, "expz", expz)
        monkeypatch.setattr(DensityProgram, "vjp", vjp)


@pytest.mark.parametrize("noise", [NoiseModel(kind="amplitude", gamma=0.1),
                                   NoiseModel(kind="amplitude", gamma=0.1, p01=0.02, p10=0.05),
                                   NoiseModel(px=0.02, py=0.02, pz=0.02, kind="depolarizing", p=0.06)])
def test_engine_adjoint_equals_param_shift_without_the_shifted_evolutions(noise, monkeypatch):
    spec, eng, x, y, w, params = _engine_setup(noise)
    cnt = _Count(monkeypatch)
    ra = eng.loss_and_grads(x, y, w, params, "adjoint")
    assert (cnt.expz, cnt.vjp) == (0, 6)                  # one forward + one backward sweep per sample
    rs = eng.loss_and_grads(x, y, w, params, "param_shift")
    assert cnt.expz == (2 * spec.n_theta + 1) * 6 and cnt.vjp == 6
    assert (ra["grad"] - rs["grad"]).abs().max() < 1e-6
    assert torch.equal(ra["loss"], rs["loss"]) and torch.equal(ra["expz"], rs["expz"])
    assert torch.equal(ra["correct"], rs["correct"])
    assert torch.equal(eng.loss_and_grads(x, y, w, params, "autograd")["grad"], ra["grad"])
    eng._budget = 2 * eng.prog.tape_bytes(spec.n_theta)   # three chunks of two rows: dL/d<Z> formed chunk by chunk
    rk = eng.loss_and_grads(x, y, w, params, "adjoint")
    assert (rk["grad"] - rs["grad"]).abs().max() < 1e-6 and torch.equal(rk["loss"], ra["loss"])
    eng._budget = eng.prog.tape_bytes(spec.n_theta) - 1
    with pytest.raises(ValueError, match="budget"):
        eng.loss_and_grads(x, y, w, params, "adjoint")


def test_shots_and_the_switch_keep_the_shift_route(monkeypatch):
    nm = NoiseModel(kind="amplitude", gamma=0.1, shots=64, seed=3)
    spec, eng, x, y, w, params = _engine_setup(nm)
    keys = nm.client_keys("shots", 0, range(2), "cpu")
    cnt = _Count(monkeypatch)
    ra = eng.loss_and_grads(x, y, w, params, "adjoint", readout_keys=keys, step=2)
    assert cnt.vjp == 0 and cnt.expz == (2 * spec.n_theta + 1) * 6
    rs = eng.loss_and_grads(x, y, w, params, "param_shift", readout_keys=keys, step=2)
    assert torch.equal(ra["grad"], rs["grad"])
    # the switch restores the substitution for exact readouts as well
    spec, eng, x, y, w, params = _engine_setup(NoiseModel(kind="amplitude", gamma=0.1))
    monkeypatch.setenv("QFEDX_DM_ADJOINT", "0")
    cnt.expz = cnt.vjp = 0
    ra = eng.loss_and_grads(x, y, w, params, "adjoint")
    assert cnt.vjp == 0 and cnt.expz == (2 * spec.n_theta + 1) * 6
    assert torch.equal(ra["grad"], eng.loss_and_grads(x, y, w, params, "param_shift")["grad"])


def test_amplitude_noise_federated_run_trains_through_the_reverse_sweep(monkeypatch):
    from qfedx_amd.api import run_experiment
    from tests.test_fl import small_cfg
    cfg = small_cfg(num_rounds=3, kind="vqc", n_qubits=4, n_layers=1, num_clients=2, samples_per_client=24,
                    batch_size=12, optimizer="sgd")
    cfg.noise.kind, cfg.noise.gamma = "amplitude", 0.05
    assert cfg.train.grad_method == "adjoint"            # the config default
    cnt = _Count(monkeypatch)
    out = run_experiment(cfg)
    assert out["simulator"] == "density" and cnt.vjp > 0
    assert len(out["accuracies"]) == 4 and all(np.isfinite(out["accuracies"]))
    assert all(np.isfinite(h["train_loss"]) for h in out["history"] if "train_loss" in h)


def test_chunked_vjp_is_bitwise_the_unchunked_one(monkeypatch):
    prog, rows, w, n_grad = vqc_case(3, 2, "amplitude", 0.0, 0.2, "ring", [0, 2, 1], S=5)
    per = prog.tape_bytes(n_grad)
    assert per == 12 * 64 * 16                            # J = 2 n L gates x 4^n entries x complex128 on the CPU
    z0, g0 = prog.vjp(rows, w, n_grad)
    calls = []
    fn = prog._vjp_torch
    monkeypatch.setattr(prog, "_vjp_torch", lambda r, *a: calls.append(r.shape[0]) or fn(r, *a))
    z1, g1 = prog.vjp(rows, w, n_grad, budget=2 * per + 7)
    assert calls == [2, 2, 1]
    assert torch.equal(z0, z1) and torch.equal(g0, g1)
    z2, g2 = prog.vjp(rows, lambda z, lo, hi: w[lo:hi], n_grad, budget=per)     # callable weights, chunks of one
    assert calls[3:] == [1] * 5 and torch.equal(z0, z2) and torch.equal(g0, g2)
    with pytest.raises(ValueError, match=f"budget of {per - 1} bytes"):
        prog.vjp(rows, w, n_grad, budget=per - 1)
    monkeypatch.setenv("QFEDX_DM_TAPE_MB", str(3 * per / (1 << 20)))            # the override wins over the argument
    del calls[:]
    z3, g3 = prog.vjp(rows, w, n_grad, budget=per - 1)
    assert calls == [3, 2] and torch.equal(z0, z3) and torch.equal(g0, g3)
