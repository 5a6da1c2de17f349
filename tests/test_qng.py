"""Quantum natural gradient: the float64 metric oracle (vs the fidelity Hessian), the reference step, the refusals and
the federated run (CPU)."""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from qfedx_amd.config import load_config
from qfedx_amd.fl.optim import BatchedOptimizer
from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import qng
from qfedx_amd.ops.engine import VQCEngine
from qfedx_amd.ops.statevec_torch import TorchProgram
from tests.test_fl import small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(spec, K, B, seed=0, theta_std=0.7):
    """(xang [K, B, x_width] float64, theta [K, n_theta] float64, init or None)."""
    g = torch.Generator().manual_seed(seed)
    theta = torch.randn(K, spec.n_theta, generator=g, dtype=torch.float64) * theta_std
    if spec.amplitude:
        init = torch.randn(K, B, 1 << spec.n_qubits, generator=g, dtype=torch.float64)
        return torch.zeros(K, B, 1, dtype=torch.float64), theta, init
    return torch.rand(K, B, spec.n_qubits, generator=g, dtype=torch.float64) * math.pi, theta, None


def _final_states(spec, xang, theta, init):
    """The circuit's final states [K * B, 2^n] in complex128, gates in the order the circuit emits them."""
    ops, coef = spec.program()
    K, B, _ = xang.shape
    prog = TorchProgram(ops, coef, spec.n_qubits, "cpu", torch.complex128)
    rows = torch.cat([theta[:, None, :].expand(K, B, -1), xang], -1).reshape(K * B, -1)
    st = None
    if init is not None:
        st = spec.initial_states(init).reshape(K * B, -1).to(torch.complex128)
        st = st / st.abs().pow(2).sum(-1, keepdim=True).sqrt()
    return prog.run(rows, state=st)


# ------------------------------------------------------------------------------------------------ 1. fidelity Hessian
@pytest.mark.parametrize("layers,entangler,fmap", [(2, "chain", "ry"), (2, "ring", "ry"), (1, "chain", "amplitude")])
def test_blocks_are_minus_half_the_fidelity_hessian(layers, entangler, fmap):
    """g = -1/2 d^2 |<psi(theta)|psi(theta + d)>|^2 / dd_i dd_j at d = 0, central differences (h = 1e-4, float64).  The
    difference quotient's own error is h^2 truncation (~1e-8) plus rounding 1e-16 / h^2 = 1e-8: bound 1e-6."""
    spec = VQCSpec(n_qubits=3, n_layers=layers, n_classes=2, feature_map=fmap, entangler=entangler)
    xang, theta, init = _inputs(spec, 1, 2, seed=3)
    G = qng.fubini_study_blocks(spec, xang, theta, init)           # [1, 2, 2L, 3, 3]
    assert G.shape == (1, 2, 2 * layers, 3, 3) and G.dtype == torch.float64
    psi0 = _final_states(spec, xang, theta, init)
    h = 1e-4
    slots = qng.block_slots(spec)

    def fid(delta):
        psi = _final_states(spec, xang, theta + delta[None, :], init)
        return (psi0.conj() * psi).sum(-1).abs() ** 2               # [B]

    worst = 0.0
    for b in range(2 * layers):
        for i in range(3):
            for j in range(i, 3):
                ei = torch.zeros(spec.n_theta, dtype=torch.float64)
                ej = torch.zeros(spec.n_theta, dtype=torch.float64)
                ei[slots[b, i]] = h
                ej[slots[b, j]] = h
                hess = (fid(ei + ej) - fid(ei - ej) - fid(ej - ei) + fid(-ei - ej)) / (4 * h * h)
                err = (G[0, :, b, i, j] + 0.5 * hess).abs().max().item()
                worst = max(worst, err)
    print(f"qng hessian check {layers}L {entangler} {fmap}: max err {worst:.3e}")
    assert worst < 1e-6


# ------------------------------------------------------------------------------------------------ 2. structure
@pytest.mark.parametrize("entangler,fmap", [("chain", "ry"), ("ring", "rx"), ("none", "rz"), ("chain", "amplitude")])
def test_block_structure(entangler, fmap):
    spec = VQCSpec(n_qubits=4, n_layers=2, n_classes=3, feature_map=fmap, entangler=entangler)
    xang, theta, init = _inputs(spec, 2, 3, seed=5)
    G = qng.fubini_study_blocks(spec, xang, theta, init)
    assert torch.equal(G, G.transpose(-1, -2))
    assert torch.linalg.eigvalsh(G).min().item() >= -1e-12
    assert G.abs().max().item() <= 0.25 + 1e-15
    d = torch.diagonal(G, dim1=-2, dim2=-1)
    assert d.min().item() >= 0.0 and d.max().item() <= 0.25
    # the diagonal is 1/4 (1 - <K>^2): <Z_i> of the RZ blocks read off the state behind the layer's RX gates
    ops, coef = spec.program()
    seg = qng.metric_segments(spec)
    prog = TorchProgram(ops, coef, 4, "cpu", torch.complex128)
    rows = torch.cat([theta[:, None, :].expand(2, 3, -1), xang], -1).reshape(6, -1)
    st = prog.initial_state(6)
    if init is not None:
        st = spec.initial_states(init).reshape(6, -1).to(torch.complex128)
        st = st / st.abs().pow(2).sum(-1, keepdim=True).sqrt()
    ang = prog.angles(rows)
    for g in seg["feature"] + seg["rx"][0]:
        st = prog.apply_gate(st, g, ang[:, g])
    z = prog.expz(st, range(4))
    assert torch.allclose(d.reshape(6, 4, 4)[:, 1], 0.25 * (1 - z ** 2), atol=1e-14, rtol=0)


def test_first_rx_block_of_a_product_state_is_diagonal_cos2():
    spec = VQCSpec(n_qubits=4, n_layers=1, n_classes=2, feature_map="ry")
    xang, theta, _ = _inputs(spec, 2, 3, seed=7)
    G = qng.fubini_study_blocks(spec, xang, theta)[:, :, 0]        # RX block of layer 1: psi = prod RY(x_i)|0>
    want = torch.diag_embed(0.25 * torch.cos(xang) ** 2)
    assert torch.allclose(G, want, atol=1e-14, rtol=0)


def test_zero_angle_rz_block_on_the_zero_state_is_exactly_zero():
    spec = VQCSpec(n_qubits=3, n_layers=2, n_classes=2, feature_map="ry")
    G = qng.fubini_study_blocks(spec, torch.zeros(1, 2, 3, dtype=torch.float64),
                                torch.zeros(1, spec.n_theta, dtype=torch.float64))
    assert torch.equal(G[:, :, 1::2], torch.zeros_like(G[:, :, 1::2]))
    assert torch.allclose(G[:, :, 0], 0.25 * torch.eye(3, dtype=torch.float64).expand(1, 2, 3, 3))


def test_client_metric_is_the_mean_over_live_samples_and_zero_without_one():
    spec = VQCSpec(n_qubits=3, n_layers=1, n_classes=2)
    xang, theta, _ = _inputs(spec, 2, 3, seed=9)
    params = torch.cat([theta, torch.ones(2, 4, dtype=torch.float64)], -1).float()
    w = torch.tensor([[0.5, 0.0, 0.5], [0.0, 0.0, 0.0]])
    eng = VQCEngine(spec, "cpu", "torch")
    G = eng.metric_blocks(xang.float(), w, params)
    per = qng.fubini_study_blocks(spec, xang.float(), params[:, :spec.n_theta])
    assert G.shape == (2, 2, 3, 3) and G.dtype == torch.float64
    assert torch.allclose(G[0], 0.5 * (per[0, 0] + per[0, 2]), atol=1e-15, rtol=0)
    assert torch.equal(G[1], torch.zeros_like(G[1]))


# ------------------------------------------------------------------------------------------------ 3. the step
def _step_case(n=3, L=2, K=3, seed=11):
    spec = VQCSpec(n_qubits=n, n_layers=L, n_classes=2)
    g = torch.Generator().manual_seed(seed)
    params = torch.randn(K, spec.n_params, generator=g)
    grad = torch.randn(K, spec.n_params, generator=g)
    A = torch.randn(K, 2 * L, n, n, generator=g, dtype=torch.float64)
    G = A @ A.transpose(-1, -2) / (4 * n)
    G[1, 2] = 0.0                                                   # an exactly singular block: damping alone
    active = torch.tensor([1.0, 1.0, 0.0][:K])
    return spec, params, grad, G, active


@pytest.mark.parametrize("via", ["ref", "optimizer"])
def test_step_matches_an_explicit_per_block_solve(via):
    spec, params, grad, G, active = _step_case()
    lr, lam = 0.05, 1e-3
    n, L, K = spec.n_qubits, spec.n_layers, params.shape[0]
    want = params.double().clone()
    for k in range(K):
        if active[k] == 0:
            continue
        for b in range(2 * L):
            idx = [2 * (n * (b // 2) + i) + (b & 1) for i in range(n)]
            A = G[k, b] + lam * torch.eye(n, dtype=torch.float64)
            want[k, idx] -= lr * (torch.linalg.inv(A) @ grad[k, idx].double())
        want[k, spec.n_theta:] -= lr * grad[k, spec.n_theta:].double()
    before = params.clone()
    if via == "ref":
        qng.qng_step_ref(params, grad, G, active, lr, lam, spec)
    else:
        opt = BatchedOptimizer("qng", params.shape, "cpu", lr, backend="torch", damping=lam, spec=spec)
        opt.step(params, grad, active, metric=G)
    # one float32 rounding of the float64 result (2^-24 relative: the singular block moves by ~lr / lambda); the
    # inverse-vs-solve difference in float64 is ~1e-16 x cond <= 1e-12
    assert torch.allclose(params.double(), want, atol=1e-10, rtol=6.1e-8)
    assert torch.equal(params[2], before[2])                        # the inactive row keeps its bits
    assert not torch.equal(params[0], before[0])
    # the singular block moved by lr grad / lambda
    idx = [2 * (n * 1 + i) + 0 for i in range(n)]
    assert torch.allclose(params[1, idx].double(), before[1, idx].double() - lr / lam * grad[1, idx].double(),
                          atol=1e-4, rtol=0)


def test_optimizer_keeps_no_state_between_steps():
    spec, params, grad, G, active = _step_case()
    opt = BatchedOptimizer("qng", params.shape, "cpu", 0.05, backend="torch", spec=spec)
    a = params.clone()
    opt.step(a, grad, active, metric=G)
    opt.step(a, grad, active, metric=G)
    b = params.clone()
    for _ in range(2):
        BatchedOptimizer("qng", params.shape, "cpu", 0.05, backend="torch", spec=spec).step(b, grad, active, metric=G)
    assert torch.equal(a, b)


@pytest.mark.parametrize("lam", [0.0, -1e-3])
def test_nonpositive_damping_raises(lam):
    spec, params, grad, G, active = _step_case()
    with pytest.raises(ValueError, match="qng_damping"):
        qng.qng_step_ref(params, grad, G, active, 0.05, lam, spec)
    with pytest.raises(ValueError, match="qng_damping"):
        BatchedOptimizer("qng", params.shape, "cpu", 0.05, backend="torch", damping=lam, spec=spec)


def test_step_without_a_metric_raises():
    spec, params, grad, G, active = _step_case()
    with pytest.raises(ValueError, match="metric"):
        BatchedOptimizer("qng", params.shape, "cpu", 0.05, backend="torch", spec=spec).step(params, grad, active)


# ------------------------------------------------------------------------------------------------ 4. refusals
def _runner(cfg):
    from qfedx_amd.api import setup
    from qfedx_amd.data.datasets import build_federated_data
    from qfedx_amd.fl.adapters import make_adapter
    from qfedx_amd.fl.server import FederatedRunner
    from qfedx_amd.parallel.dist import shard_clients
    device, backend, world = setup(cfg)
    data = build_federated_data(cfg, clients=shard_clients(cfg.data.num_clients, world.world_size, world.rank))
    return FederatedRunner(cfg, make_adapter(cfg, device, backend), data, world, device, backend)


@pytest.mark.parametrize("kw,key", [
    ({"noise.kind": "depolarizing", "noise.p": 0.01}, "noise.kind"),
    ({"noise.kind": "amplitude_twirl", "noise.gamma": 0.01}, "noise.kind"),
    ({"model.simulator": "mps"}, "model.simulator"),
    ({"model.simulator": "density"}, "model.simulator"),
    ({"privacy.dp": True, "privacy.level": "record"}, "privacy.level"),
    ({"model.n_qubits": 33}, "model.n_qubits"),
    ({"model.n_qubits": 28}, "model.n_qubits"),                     # two 2 GiB states pass the CPU state budget
    ({"train.qng_damping": 0.0}, "train.qng_damping"),
    ({"train.qng_damping": -1.0}, "train.qng_damping"),
    ({"model.kind": "tinycnn"}, "model.kind"),
])
def test_forbidden_combinations_raise_naming_the_key(kw, key):
    cfg = small_cfg(num_rounds=1, **{"train.optimizer": "qng", **kw})
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        _runner(cfg)


def test_engine_refuses_a_budget_below_two_states():
    spec = VQCSpec(n_qubits=4, n_layers=1, n_classes=2)
    eng = VQCEngine(spec, "cpu", "torch")
    eng._budget = 2 * 8 * 16 - 1
    with pytest.raises(ValueError, match="model.n_qubits"):
        eng.metric_blocks(torch.zeros(1, 2, 4), torch.ones(1, 2), spec.init_params(0)[None])


@pytest.mark.parametrize("method", ["adjoint", "param_shift", "autograd"])
def test_every_gradient_method_is_allowed(method):
    from qfedx_amd.api import run_experiment
    out = run_experiment(small_cfg(num_rounds=1, **{"train.optimizer": "qng", "train.grad_method": method}))
    assert torch.isfinite(out["params"]).all()


# ------------------------------------------------------------------------------------------------ 5. federated runs
def test_iris_qng_run():
    cfg = load_config(os.path.join(ROOT, "configs", "iris_4q_qng.yaml"),
                      ["train.num_rounds=3", "runtime.device=cpu", "runtime.log_every=100"])
    assert cfg.train.optimizer == "qng" and cfg.train.qng_damping == 1e-3
    runner = _runner(cfg)
    start = runner.params.clone()
    out = runner.run()
    assert torch.isfinite(out["params"]).all() and not torch.equal(out["params"].cpu(), start.cpu())
    hist = [h for h in out["history"] if "train_loss" in h]
    assert len(hist) == 3 and all(math.isfinite(h["train_loss"]) for h in hist)


def test_qng_keeps_client_level_dp_and_secure_agg():
    from qfedx_amd.api import run_experiment
    out = run_experiment(small_cfg(num_rounds=2, dp=True, secure_agg=True, deterministic_noise=True,
                                   **{"train.optimizer": "qng"}))
    assert torch.isfinite(out["params"]).all() and out["history"][-1]["epsilon"] > 0


def test_qng_round_differs_from_plain_sgd_and_is_reproducible():
    from qfedx_amd.api import run_experiment
    a = run_experiment(small_cfg(num_rounds=1, **{"train.optimizer": "qng"}))["params"]
    a2 = run_experiment(small_cfg(num_rounds=1, **{"train.optimizer": "qng"}))["params"]
    b = run_experiment(small_cfg(num_rounds=1, **{"train.optimizer": "sgd", "train.momentum": 0.0}))["params"]
    assert torch.equal(a, a2) and not torch.equal(a, b)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, kw, out_path):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from qfedx_amd.api import run_experiment
    out = run_experiment(small_cfg(**kw))
    if rank == 0:
        torch.save({"params": out["params"]}, out_path)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_two_ranks_bitwise_equal_single_process(tmp_path):
    """A client's metric and step depend on its own samples only: 1 and 2 ranks give the same model bit for bit."""
    from qfedx_amd.api import run_experiment
    kw = {"num_rounds": 2, "num_clients": 5, "train.optimizer": "qng", "client_fraction": 0.8}
    single = run_experiment(small_cfg(**kw))
    out_path = str(tmp_path / "out2.pt")
    mp.spawn(_worker, args=(2, _free_port(), kw, out_path), nprocs=2, join=True)
    two = torch.load(out_path, weights_only=True)
    assert torch.equal(two["params"], single["params"])
