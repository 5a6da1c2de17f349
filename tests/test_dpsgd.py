"""Record-level DP-SGD (privacy.level: record): the float64 reference step, the torch engine's per-sample path, Poisson
lots, the server wiring and the accounting.  CPU only; the device reductions are tests/test_gpu_dpsgd.py."""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from qfedx_amd.config import load_config
from qfedx_amd.fl.trainer import BatchPlan, lot_width
from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops.engine import VQCEngine
from qfedx_amd.privacy import accountant
from qfedx_amd.privacy.dp import dpsgd_noise, dpsgd_step_ref
from qfedx_amd.utils.seeding import philox_key, philox_normal
from tests.test_fl import small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- dpsgd_step_ref
def _rows(K=3, B=5, P=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    grads = torch.randn(K, B, P, generator=g, dtype=torch.float64) * torch.logspace(-1, 1, B, dtype=torch.float64)[None, :, None]
    keys = torch.tensor([philox_key(11, "dpsgd_noise", 2, k) for k in range(K)], dtype=torch.int64)
    return grads, keys


def test_ref_no_noise_huge_clip_is_the_plain_sum():
    g, keys = _rows()
    live = torch.ones(3, 5)
    live[1, 2:] = 0
    out = dpsgd_step_ref(g, live, 1e30, 0.0, keys, 0, 8)
    assert torch.equal(out["c"], torch.ones(3, 5, dtype=torch.float64))
    # sum over the live rows / lot = the live rows' mean gradient x (live / lot)
    n = live.sum(-1).double()
    mean = (g * live[..., None]).sum(1) / n[:, None]
    assert torch.allclose(out["grad"], mean * (n / 8)[:, None], rtol=1e-14, atol=0)


def test_ref_clipped_rows_have_norm_at_most_c():
    g, keys = _rows()
    C = float(g.norm(dim=-1).median())
    out = dpsgd_step_ref(g, torch.ones(3, 5), C, 0.0, keys, 0, 5)
    clipped = g * out["c"][..., None]
    assert (clipped.norm(dim=-1) <= C * (1 + 1e-12)).all()
    assert (out["c"] < 1).any() and (out["c"] == 1).any()
    assert torch.equal(out["norm"], g.norm(dim=-1))


def test_ref_weight_zero_row_contributes_nothing():
    g, keys = _rows()
    live = torch.ones(3, 5)
    live[0, 3] = 0
    a = dpsgd_step_ref(g, live, 1.0, 0.7, keys, 3, 5)
    g2 = g.clone()
    g2[0, 3] = 1e6                       # whatever the masked row holds
    b = dpsgd_step_ref(g2, live, 1.0, 0.7, keys, 3, 5)
    assert torch.equal(a["grad"], b["grad"])


def test_ref_empty_lot_is_exactly_the_noise():
    g, keys = _rows()
    sigma, C, lot, step = 1.3, 0.5, 8, 2
    out = dpsgd_step_ref(g, torch.zeros(3, 5), C, sigma, keys, step, lot)
    for k in range(3):
        z = dpsgd_noise(7, keys[k].tolist(), step).double()
        assert torch.equal(out["grad"][k], sigma * C * z / lot)
    assert torch.equal(dpsgd_step_ref(g, torch.zeros(3, 5), C, 0.0, keys, step, lot)["grad"], torch.zeros(3, 7, dtype=torch.float64))


@pytest.mark.parametrize("P,step", [(7, 0), (7, 1), (7, 3), (10, 5), (4, 2)])
def test_ref_noise_is_philox_normal_at_step_offsets(P, step):
    key = philox_key(5, "dpsgd_noise", 1, 9)
    stream = philox_normal((step + 1) * P, key)
    assert torch.equal(dpsgd_noise(P, key, step), stream[step * P:(step + 1) * P])


# ---------------------------------------------------------------------------------------------- torch engine
@pytest.mark.parametrize("method", ["adjoint", "autograd"])
def test_torch_engine_dpsgd_matches_reference_on_autograd_rows(method):
    spec = VQCSpec(n_qubits=4, n_layers=2, n_classes=3)
    eng = VQCEngine(spec, "cpu", "torch")
    K, B = 2, 5
    g = torch.Generator().manual_seed(3)
    xang = spec.encode_features(torch.rand(K, B, 4, generator=g))
    y = torch.randint(0, 3, (K, B), generator=g)
    w = torch.full((K, B), 1.0 / B)
    w[1, 4] = 0                                     # one row outside the lot
    params = torch.stack([spec.init_params(k) for k in range(K)]) + 0.3 * torch.randn(K, spec.n_params, generator=g)
    keys = torch.tensor([philox_key(7, "dpsgd_noise", 0, k) for k in range(K)], dtype=torch.int64)
    # per-sample gradients by plain autograd: one evaluation per (client, sample) with unit weight
    rows = torch.zeros(K, B, spec.n_params, dtype=torch.float64)
    for k in range(K):
        for b in range(B):
            r = eng.loss_and_grads(xang[k:k + 1, b:b + 1], y[k:k + 1, b:b + 1], torch.ones(1, 1), params[k:k + 1], "autograd")
            rows[k, b] = r["grad"][0].double()
    C = float(rows.norm(dim=-1).median())
    for sigma in (0.0, 1.0):
        dp = dict(clip=C, sigma=sigma, keys=keys, step=2, lot=4)
        ref = dpsgd_step_ref(rows, w, C, sigma, keys, 2, 4)
        out = eng.loss_and_grads(xang, y, w, params, method, dpsgd=dp)
        assert "opt_done" not in out
        scale = float(ref["grad"].abs().max())
        assert (out["grad"].double() - ref["grad"]).abs().max() <= 2e-6 * scale      # float32 rows and results
        on = w > 0                                  # (the engine never forms the gradient of a row outside the lot)
        assert torch.allclose(out["dp_norm"][on], ref["norm"][on], rtol=1e-5)
        assert (out["dp_c"][on] < 1).any() and (out["dp_c"][on] == 1).any()
    plain = eng.loss_and_grads(xang, y, (w > 0).float() / (w > 0).sum(-1, keepdim=True), params, "adjoint")
    assert torch.allclose(out["loss"], plain["loss"], atol=1e-6)            # mean CE over the live samples
    assert torch.equal(out["correct"], plain["correct"])


def test_engine_refuses_methods_without_per_sample_gradients():
    spec = VQCSpec(n_qubits=4, n_layers=1, n_classes=2)
    eng = VQCEngine(spec, "cpu", "torch")
    x = spec.encode_features(torch.rand(1, 2, 4))
    y = torch.zeros(1, 2, dtype=torch.int64)
    p = spec.init_params(0)[None]
    dp = dict(clip=1.0, sigma=0.0, keys=None, step=0, lot=2)
    for method in ("param_shift", "spsa"):
        with pytest.raises(ValueError, match="grad_method"):
            eng.loss_and_grads(x, y, torch.ones(1, 2), p, method, dpsgd=dp)
    for backend in ("mps", "density"):
        e2 = VQCEngine(spec, "cpu", backend)
        with pytest.raises(ValueError, match="simulator"):
            e2.loss_and_grads(x, y, torch.ones(1, 2), p, "adjoint", dpsgd=dp)


# ---------------------------------------------------------------------------------------------- Poisson lots
def _lots(counts, ids, B=8, rnd=3, **kw):
    return BatchPlan(torch.tensor(counts), ids, B, rnd, 99, poisson={"seed": 4242, **kw.pop("poisson", {})}, **kw)


def test_poisson_lots_do_not_depend_on_the_rank_layout():
    counts, ids = [40, 23, 64, 5, 31], [0, 1, 2, 3, 4]
    nmax = max(counts)
    full = _lots(counts, ids, local_steps=3, poisson={"nmax": nmax})
    assert full.B == lot_width(8, nmax) == min(nmax, 8 + math.ceil(6 * math.sqrt(8)))
    assert tuple(full.idx.shape) == (3, 5, full.B) and tuple(full.wts.shape) == (3, 5, full.B)
    for sub in ([0, 2, 4], [1, 3], [4], [3, 0]):
        part = _lots([counts[i] for i in sub], sub, local_steps=3, poisson={"nmax": nmax})
        assert torch.equal(part.idx, full.idx[:, sub]) and torch.equal(part.wts, full.wts[:, sub])
        assert torch.equal(part.active, full.active[:, sub])
    assert set(full.wts.unique().tolist()) <= {0.0, 1.0}
    # every live index is a record of its client; no record twice in a lot
    for k, n in enumerate(counts):
        for s in range(3):
            live = full.idx[s, k][full.wts[s, k] > 0]
            assert (live < n).all() and live.unique().numel() == live.numel()
    assert full.overflow == 0
    other = _lots(counts, ids, rnd=4, local_steps=3, poisson={"nmax": nmax})
    assert not torch.equal(other.wts, full.wts) or not torch.equal(other.idx, full.idx)     # keyed by the round


def test_poisson_q_one_clients_draw_their_whole_shard():
    plan = _lots([5, 8, 40], [7, 8, 9], B=8, local_epochs=2)
    assert plan.q.tolist() == [1.0, 1.0, 0.2]
    assert plan.steps_per_client == [2, 2, 10]             # local_epochs x ceil(n / B), as without DP
    for k, n in ((0, 5), (1, 8)):
        for s in range(2):
            live = plan.idx[s, k][plan.wts[s, k] > 0]
            assert sorted(live.tolist()) == list(range(n))
        assert plan.wts[2:, k].sum() == 0 and plan.active[2:, k].sum() == 0       # past their step budget


def test_poisson_overflow_drops_by_priority_and_counts():
    big = _lots([30], [3], B=8, local_steps=4, poisson={"nmax": 30})
    small = _lots([30], [3], B=8, local_steps=4, poisson={"nmax": 30, "bcap": 3})
    assert small.B == 3 and tuple(small.idx.shape) == (4, 1, 3)
    sizes = (big.wts > 0).sum(-1)[:, 0]
    assert (sizes > 3).any()                                # the case is an overflow
    assert small.overflow == int((sizes - 3).clamp(min=0).sum()) > 0
    for s in range(4):
        # live rows come in priority order: the capped lot is the first Bcap of the full one
        n = min(3, int(sizes[s]))
        assert torch.equal(small.idx[s, 0, :n], big.idx[s, 0, :n]) and small.wts[s, 0, :n].sum() == n
        assert small.wts[s, 0, n:].sum() == 0


def test_poisson_inclusion_count_is_binomial():
    plan = _lots([64], [0], B=16, local_steps=200)          # q = 0.25, 200 steps, fixed key
    total = int(plan.wts.sum())
    sd = math.sqrt(200 * 64 * 0.25 * 0.75)
    assert plan.overflow == 0 and abs(total - 3200) <= 5 * sd, total
    per_record = torch.zeros(64)
    for s in range(200):
        per_record[plan.idx[s, 0][plan.wts[s, 0] > 0]] += 1
    assert (per_record - 50).abs().max() <= 5 * math.sqrt(200 * 0.25 * 0.75)


# ---------------------------------------------------------------------------------------------- server
def _runner(cfg):
    from qfedx_amd.api import setup
    from qfedx_amd.data.datasets import build_federated_data
    from qfedx_amd.fl.adapters import make_adapter
    from qfedx_amd.fl.server import FederatedRunner
    from qfedx_amd.parallel.dist import shard_clients
    device, backend, world = setup(cfg)
    data = build_federated_data(cfg, clients=shard_clients(cfg.data.num_clients, world.world_size, world.rank))
    return FederatedRunner(cfg, make_adapter(cfg, device, backend), data, world, device, backend)


def test_iris_record_level_run_reports_record_epsilon(monkeypatch):
    cfg = load_config(os.path.join(ROOT, "configs", "iris_4q_dpsgd.yaml"),
                      ["train.num_rounds=2", "runtime.device=cpu", "runtime.log_every=100"])
    assert cfg.privacy.dp and cfg.privacy.level == "record"
    import qfedx_amd.fl.aggregator as agg

    def boom(*a, **k):
        raise AssertionError("the aggregator clipped / noised a client update under privacy.level=record")
    monkeypatch.setattr(agg, "clip_and_noise", boom)
    runner = _runner(cfg)
    assert runner.aggregator.dp is False and runner.record_dp and not runner.client_dp
    out = runner.run()
    counts = runner.store.counts
    B = cfg.train.batch_size
    q_max = min(1.0, B / int(counts.min()))
    steps = cfg.train.local_epochs * math.ceil(int(counts.max()) / B)
    assert runner.dp_q_max == q_max and runner.dp_round_steps == steps
    hist = [h for h in out["history"] if "epsilon" in h]
    assert len(hist) == 2
    for i, h in enumerate(hist):
        assert h["dp_level"] == "record" and h["dp_lot_overflow"] == 0
        assert h["epsilon"] == accountant.epsilon(q_max, cfg.privacy.noise_multiplier, (i + 1) * steps, cfg.privacy.delta)
        assert math.isfinite(h["train_loss"])
    assert out["epsilon"] == hist[-1]["epsilon"] > 0


def test_default_level_is_client_and_records_are_unchanged():
    from qfedx_amd.api import run_experiment
    out = run_experiment(small_cfg(num_rounds=1, dp=True, deterministic_noise=True))
    assert "dp_level" not in out["history"][-1] and "dp_lot_overflow" not in out["history"][-1]
    assert small_cfg().privacy.level == "client"


@pytest.mark.parametrize("kw,key", [
    ({"noise_mode": "distributed", "secure_agg": True, "weighting": "uniform"}, "privacy.noise_mode"),
    ({"grad_method": "param_shift"}, "train.grad_method"),
    ({"grad_method": "spsa"}, "train.grad_method"),
    ({"noise.kind": "depolarizing", "noise.p": 0.01}, "noise.kind"),
    ({"noise.readout_p01": 0.02}, "noise.kind"),
    ({"model.simulator": "mps"}, "model.simulator"),
    ({"model.kind": "tinycnn"}, "model.kind"),
    ({"privacy.level": "sample"}, "privacy.level"),
])
def test_forbidden_combinations_raise_naming_the_key(kw, key):
    cfg = small_cfg(num_rounds=1, dp=True, **{"privacy.level": "record", **kw})
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        _runner(cfg)


def test_record_level_keeps_secure_agg():
    from qfedx_amd.api import run_experiment
    out = run_experiment(small_cfg(num_rounds=1, dp=True, secure_agg=True, deterministic_noise=True,
                                   **{"privacy.level": "record"}))
    assert out["history"][-1]["dp_level"] == "record" and torch.isfinite(out["params"]).all()


def test_record_level_noise_changes_with_the_round_and_sigma():
    """sigma = 0 is deterministic in the lots alone; sigma > 0 moves the model; the run is reproducible."""
    from qfedx_amd.api import run_experiment
    kw = dict(num_rounds=2, dp=True, deterministic_noise=True, **{"privacy.level": "record"})
    a = run_experiment(small_cfg(noise_multiplier=0.0, **kw))["params"]
    b = run_experiment(small_cfg(noise_multiplier=1.0, **kw))["params"]
    b2 = run_experiment(small_cfg(noise_multiplier=1.0, **kw))["params"]
    assert torch.equal(b, b2) and not torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- rank invariance
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
        torch.save({"params": out["params"], "eps": torch.tensor([h["epsilon"] for h in out["history"]], dtype=torch.float64)}, out_path)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_two_ranks_bitwise_equal_single_process(tmp_path):
    """Lots and noise are keyed by (seed, round, client, step), q_max and the lot width are agreed over ranks: 1 and 2
    ranks give the same model bit for bit (uneven shards: non-IID partition)."""
    from qfedx_amd.api import run_experiment
    kw = {"num_rounds": 2, "num_clients": 5, "dp": True, "deterministic_noise": True, "privacy.level": "record",
          "noise_multiplier": 0.8, "client_fraction": 0.8}
    single = run_experiment(small_cfg(**kw))
    out_path = str(tmp_path / "out2.pt")
    mp.spawn(_worker, args=(2, _free_port(), kw, out_path), nprocs=2, join=True)
    two = torch.load(out_path, weights_only=True)
    assert torch.equal(two["params"], single["params"])
    assert two["eps"].tolist() == [h["epsilon"] for h in single["history"]]
