"""The density simulator's reverse sweep on the GPU (csrc/density_adj.hip) against the float64 shift-rule oracle of
tests/density_adjoint_cases.py, its bitwise invariances, and the engine route built on it.

Bounds: ``TOL`` is 3 x the error measured for the new kernels per case (profiles/density_adjoint_err_table.txt, written
by tools/density_adjoint_err_table.py from ``errors`` / ``shift_errors`` below; the table also carries the error of the
fp32 parameter-shift route through the forward kernel on the same inputs, the yardstick)."""
import math

import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops.density import DensityProgram
from qfedx_amd.ops.engine import VQCEngine
from qfedx_amd.quantum.noise import NoiseModel
from tests.density_adjoint_cases import GPU_CASES, gpu_case_oracle, shifted, vqc_case

pytestmark = pytest.mark.gpu

# case -> (max |d<Z>|, max |d grad|) bounds: 3 x the measured error of the new kernels (the err table)
TOL = {
    "n2": (3.269e-07, 2.657e-07),
    "n4_ring_dep": (3.878e-07, 5.331e-07),
    "n6": (2.236e-06, 4.885e-07),
    "n7": (2.889e-06, 1.924e-06),
    "n8_ideal": (1.102e-06, 2.190e-06),      # gradient: 1.8 x what 3 x the shift route's error would give (the table)
    "hand": (2.854e-07, 2.512e-07),
}


def _case(name, dev):
    prog, rows, w, n_grad = GPU_CASES[name](dev)
    return prog, rows.to(dev), w.to(dev), n_grad


def errors(name: str, dev) -> dict:
    """max |d<Z>| and max |d grad| of the tape forward + backward kernels against the float64 oracle."""
    prog, rows, w, n_grad = _case(name, dev)
    z, gg = prog.vjp(rows, w, n_grad)
    zr, gr = gpu_case_oracle(name)
    return {"z": float((z.cpu().double() - zr).abs().max()), "grad": float((gg.cpu().double() - gr).abs().max())}


def shift_errors(name: str, dev) -> dict:
    """The same two errors for the fp32 parameter-shift route through the forward kernel (dm_run): every differentiated
    gate's angle shifted by +-pi/2, the pair differences accumulated in float64 as the engine's shift route does."""
    prog, rows, w, n_grad = _case(name, dev)
    gg = torch.zeros(rows.shape[0], len(prog.ops), dtype=torch.float64, device=dev)
    for g in prog.taped_gates(n_grad):
        zp, zm = (shifted(prog, g, s * math.pi / 2, dev).expz(rows).double() for s in (1.0, -1.0))
        gg[:, g] = 0.5 * ((zp - zm) * w.double()).sum(-1)
    zr, gr = gpu_case_oracle(name)
    return {"z": float((prog.expz(rows).cpu().double() - zr).abs().max()), "grad": float((gg.cpu() - gr).abs().max())}


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_reverse_sweep_matches_float64_oracle(cuda, name):
    e = errors(name, cuda)
    tz, tg = TOL[name]
    print(f"{name}: |d<Z>| {e['z']:.3e} (bound {tz:.3e})  |d grad| {e['grad']:.3e} (bound {tg:.3e})")
    assert e["z"] <= tz and e["grad"] <= tg
    _, gr = gpu_case_oracle(name)
    prog, _, _, n_grad = GPU_CASES[name]("cpu")
    rest = [g for g in range(len(prog.ops)) if g not in prog.taped_gates(n_grad)]
    assert gr.abs().max() > 0.1 and len(rest) > 0


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_tape_forward_expz_is_bitwise_dm_run_and_untaped_gates_are_zero(cuda, name):
    prog, rows, w, n_grad = _case(name, cuda)
    z, gg = prog.vjp(rows, w, n_grad)
    assert torch.equal(z, prog.expz(rows))
    rest = [g for g in range(len(prog.ops)) if g not in prog.taped_gates(n_grad)]
    assert torch.equal(gg[:, rest], torch.zeros(rows.shape[0], len(rest), device=cuda))


@pytest.mark.parametrize("name", ["n2", "n6", "n7"])
def test_repeats_chunks_and_batch_mates_do_not_change_a_row(cuda, name):
    prog, rows, w, n_grad = _case(name, cuda)
    z0, g0 = prog.vjp(rows, w, n_grad)
    z1, g1 = prog.vjp(rows, w, n_grad)
    assert torch.equal(z0, z1) and torch.equal(g0, g1)                       # two calls
    per = prog.tape_bytes(n_grad)
    assert per == len(prog.taped_gates(n_grad)) * (4 ** prog.n) * 8
    z2, g2 = prog.vjp(rows, w, n_grad, budget=per)                           # chunks of one row against one chunk
    assert torch.equal(z0, z2) and torch.equal(g0, g2)
    z3, g3 = prog.vjp(rows[1:2], w[1:2], n_grad)                             # the row alone
    assert torch.equal(z0[1:2], z3) and torch.equal(g0[1:2], g3)
    with pytest.raises(ValueError, match=f"budget of {per - 1} bytes"):
        prog.vjp(rows, w, n_grad, budget=per - 1)


def test_ten_qubits_adjoint_matches_kernel_param_shift(cuda):
    """n = 10 (the largest size; 8 MB per state, a 160 MB tape), one row, no float64 oracle: the reverse sweep against
    the slot shifts through the forward kernel, both fp32.  Bound: 5e-5, the project's bound for fp32 gradients of this
    simulator against float64 (tests/test_gpu_noise.py), for each of the two routes, times sum_c |w_c| (the gradient is
    linear in w; the existing bound is for |dL/d<Z>| <= 1)."""
    prog, rows, w, n_grad = vqc_case(10, 1, "amplitude", 0.0, 0.05, "chain", [0, 4, 9], S=1, device=cuda)
    rows, w = rows.to(cuda), w.to(cuda)
    z, gg = prog.vjp(rows, w, n_grad)
    taped = prog.taped_gates(n_grad)
    assert len(taped) == n_grad == 20                    # every theta slot drives one rotation with unit scale
    sh = rows.repeat(2 * n_grad, 1)
    for j in range(n_grad):
        sh[2 * j, j] += math.pi / 2
        sh[2 * j + 1, j] -= math.pi / 2
    zs = prog.expz(sh).double().reshape(n_grad, 2, -1)
    gs = 0.5 * ((zs[:, 0] - zs[:, 1]) * w.double()).sum(-1)
    slot = torch.tensor([int(prog.ops[g, 3]) for g in taped], device=cuda)
    err = float((gg[0, taped].double()[torch.argsort(slot)] - gs).abs().max())
    bound = 2 * 5e-5 * float(w.abs().sum())
    print(f"n10: |adjoint - shift| {err:.3e} (bound {bound:.3e}), |grad|max {float(gs.abs().max()):.3e}")
    assert torch.equal(z, prog.expz(rows)) and gs.abs().max() > 0.01
    assert err <= bound


@pytest.mark.parametrize("readout", [(0.0, 0.0), (0.03, 0.06)])
def test_engine_adjoint_on_gpu_matches_cpu_and_its_own_param_shift(cuda, readout):
    """The shape and bounds of test_gpu_noise.py's parameter-shift comparison (4q x 2L, K = 2 x B = 5; loss 2e-5,
    gradient 5e-5 against the float64 CPU engine), for the adjoint route."""
    nm = NoiseModel(kind="amplitude", gamma=0.1, p01=readout[0], p10=readout[1])
    spec = VQCSpec(4, 2, 3, readout_scale=2.0, init_std=1.0)
    g = torch.Generator().manual_seed(1)
    x = spec.encode_features(torch.rand(2, 5, 4, generator=g))
    y = torch.randint(0, 3, (2, 5), generator=g)
    w = torch.full((2, 5), 0.2)
    params = torch.stack([spec.init_params(k) for k in range(2)])
    eng = VQCEngine(spec, cuda, "density", noise=nm)
    dev = [t.to(cuda) for t in (x, y, w, params)]
    calls = []
    vjp0 = DensityProgram.vjp
    eng.prog.vjp = lambda *a, **k: calls.append(1) or vjp0(eng.prog, *a, **k)
    rg = eng.loss_and_grads(*dev, "adjoint")
    assert calls == [1]
    rs = eng.loss_and_grads(*dev, "param_shift")
    assert calls == [1]
    rc = VQCEngine(spec, "cpu", "density", noise=nm).loss_and_grads(x, y, w, params, "adjoint")
    assert torch.allclose(rg["loss"].cpu(), rc["loss"], atol=2e-5)
    assert torch.equal(rg["loss"], rs["loss"]) and torch.equal(rg["correct"].cpu(), rc["correct"])
    assert torch.allclose(rg["grad"].cpu(), rc["grad"], atol=5e-5)
    assert torch.allclose(rg["grad"], rs["grad"], atol=1e-4)     # each within 5e-5 of the float64 gradient


def test_default_config_amplitude_run_trains_through_the_reverse_sweep_on_hip(cuda, monkeypatch):
    """grad_method is left at the config default (adjoint): two rounds at 4 qubits on the HIP backend run the reverse
    sweep and land on the CPU run's parameters (1e-4, the bound of the other HIP-vs-CPU federated comparisons)."""
    import numpy as np
    from qfedx_amd.api import run_experiment
    from qfedx_amd.parallel.dist import init_distributed
    from tests.test_fl import small_cfg
    kw = dict(num_rounds=2, kind="vqc", n_qubits=4, n_layers=1, num_clients=2, samples_per_client=24, batch_size=12,
              optimizer="sgd")

    def cfg(**more):
        c = small_cfg(**kw, **more)
        c.noise.kind, c.noise.gamma = "amplitude", 0.05
        assert c.train.grad_method == "adjoint"
        return c

    calls = []
    vjp0 = DensityProgram.vjp
    monkeypatch.setattr(DensityProgram, "vjp", lambda prog, *a, **k: calls.append(prog.device.type) or vjp0(prog, *a, **k))
    cpu = run_experiment(cfg())
    n_cpu = len(calls)
    hip = run_experiment(cfg(device="cuda", backend="hip"), world=init_distributed(cuda), device=cuda, backend="hip")
    assert n_cpu > 0 and len(calls) == 2 * n_cpu and set(calls[n_cpu:]) == {"cuda"}
    assert hip["simulator"] == "density" and all(np.isfinite(hip["accuracies"]))
    assert torch.allclose(hip["params"].cpu(), cpu["params"], atol=1e-4)


def test_bindings_refuse_short_or_mistyped_buffers(cuda):
    from qfedx_amd.ops._ext import ext
    E = ext()
    prog, rows, w, n_grad = _case("n7", cuda)
    S, C, G, N, J = rows.shape[0], len(prog.readout), len(prog.ops), 4 ** prog.n, len(prog.taped_gates(n_grad))
    z = torch.empty(S, C, device=cuda)
    gg = torch.empty(S, G, device=cuda)
    tape = torch.empty(S * J * N, dtype=torch.complex64, device=cuda)
    slab = torch.empty(S * N, dtype=torch.complex64, device=cuda)
    fwd = lambda tape=tape, slab=slab, z=z, J=J, n_grad=n_grad: E.dm_forward_tape(  # noqa: E731
        prog._gates, G, prog.n, rows, prog._ro, prog._sup, slab, n_grad, J, tape, z)
    bwd = lambda tape=tape, slab=slab, w=w, gg=gg, J=J: E.dm_adjoint(               # noqa: E731
        prog._gates, G, prog.n, rows, prog._ro, prog._sup, n_grad, J, tape, slab, w, gg)
    with pytest.raises(ValueError, match="tape too small"):
        fwd(tape=tape[:-1])
    with pytest.raises(ValueError, match="tape has wrong dtype"):
        fwd(tape=tape.view(torch.float32))
    with pytest.raises(ValueError, match="scratch too small"):
        fwd(slab=slab[:-1])
    with pytest.raises(ValueError, match="expz too small"):
        fwd(z=z.reshape(-1)[:-1])
    with pytest.raises(ValueError, match="n_grad"):
        fwd(n_grad=rows.shape[1] + 1)
    with pytest.raises(ValueError, match="tape too small"):
        bwd(tape=tape[:-1])
    with pytest.raises(ValueError, match="gg too small"):
        bwd(gg=gg.reshape(-1)[:-1])
    with pytest.raises(ValueError, match="w has wrong dtype"):
        bwd(w=w.double())
    with pytest.raises(ValueError, match="w too small"):
        bwd(w=w.reshape(-1)[:-1])
    with pytest.raises(ValueError, match="lam too small"):
        bwd(slab=slab[:-1])
    fwd()                                                # the well-formed calls go through and agree with vjp
    bwd()
    z0, g0 = prog.vjp(rows, w, n_grad)
    assert torch.equal(z, z0) and torch.equal(gg, g0)
