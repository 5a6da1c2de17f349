"""Quantum natural gradient against SGD and Adam (profiles/qng_step_ab.txt), in ONE process.

1. Local-step time, interleaved: per round of the A/B every optimizer's whole local step runs back to back on the same
   engine and inputs, as fl/trainer.py runs it - sgd: loss_and_grads + the SGD kernel; adam: loss_and_grads with the
   optimizer fused where the engine fuses it; qng: the metric pass (VQCEngine.metric) + loss_and_grads + qng_step - and
   the metric pass and the qng_step launch alone.  8 clients x 32 samples at 12 qubits x 2 layers and 16 x 3.
2. Loss curves: 30 federated rounds of the three on the synthetic 8-qubit task (same data, same seed, same lr).

No thresholds: the file records what was measured.

python scripts/qng_ab.py [--out profiles/qng_step_ab.txt --rounds 7 --iters 10 --curve-rounds 30 --lr 0.05]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("QFX_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def step_times(n, L, K, B, rounds, iters, lr):
    import torch
    from qfedx_amd.fl.adapters import resolve_state_dtype
    from qfedx_amd.fl.optim import BatchedOptimizer
    from qfedx_amd.models.vqc import VQCSpec
    from qfedx_amd.ops.engine import VQCEngine

    dev = torch.device("cuda", 0)
    spec = VQCSpec(n, L, 3)
    dtype = resolve_state_dtype("auto", spec, "hip", None)
    eng = VQCEngine(spec, dev, "hip", dtype)
    g = torch.Generator().manual_seed(0)
    x = spec.encode_features(torch.rand(K, B, n, generator=g)).to(dev)
    y = torch.randint(0, 3, (K, B), generator=g).to(dev)
    w = torch.full((K, B), 1.0 / B, device=dev)
    act = torch.ones(K, device=dev)
    p0 = torch.stack([spec.init_params(k) for k in range(K)]).to(dev)
    params = {k: p0.clone() for k in ("sgd", "adam", "qng")}
    opts = {k: BatchedOptimizer(k, p0.shape, dev, lr, backend="hip", spec=spec if k == "qng" else None)
            for k in params}

    def sgd():
        r = eng.loss_and_grads(x, y, w, params["sgd"], "adjoint")
        opts["sgd"].step(params["sgd"], r["grad"], act)

    def adam():
        r = eng.loss_and_grads(x, y, w, params["adam"], "adjoint", fused_opt=(opts["adam"], act))
        if not r.get("opt_done", False):
            opts["adam"].step(params["adam"], r["grad"], act)

    state = {}

    def metric():
        state["m"] = eng.metric(x, w, params["qng"])

    def qng():
        metric()
        r = eng.loss_and_grads(x, y, w, params["qng"], "adjoint")
        state["g"] = r["grad"]
        opts["qng"].step(params["qng"], r["grad"], act, metric=state["m"])

    def qng_step_kernel():
        opts["qng"].step(params["qng"], state["g"], act, metric=state["m"])

    items = {"sgd_step": sgd, "adam_step": adam, "qng_step": qng, "qng_metric_pass": metric,
             "qng_step_kernel": qng_step_kernel}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    for fn in items.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in items}
    for _ in range(rounds):
        for name, fn in items.items():
            res[name].append(timed(fn))
    out = {"qubits": n, "layers": L, "clients": K, "batch": B, "state_dtype": dtype, "rounds": rounds, "iters": iters}
    for name, v in res.items():
        out[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                     "spread_ms": round(max(v) - min(v), 4)}
    return out


def curves(rounds, lr, backend="hip"):
    from qfedx_amd.api import run_experiment
    from qfedx_amd.config import ExperimentConfig, apply_overrides
    out = {}
    for opt in ("sgd", "adam", "qng"):
        cfg = ExperimentConfig()
        apply_overrides(cfg, ["data.dataset=synthetic", "data.num_clients=8", "data.samples_per_client=64",
                              "model.n_qubits=8", "model.n_layers=2", "model.readout_scale=3.0",
                              f"train.num_rounds={rounds}", "train.batch_size=32", f"train.learning_rate={lr}",
                              f"train.optimizer={opt}", f"runtime.backend={backend}",
                              f"runtime.device={'cuda' if backend == 'hip' else 'cpu'}",
                              "runtime.log_every=1000"])
        hist = run_experiment(cfg)["history"]
        out[opt] = {"train_loss": [round(h["train_loss"], 4) for h in hist],
                    "test_loss": [round(h["test_loss"], 4) for h in hist if "test_loss" in h],
                    "test_acc": [round(h["test_acc"], 4) for h in hist if "test_acc" in h]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "qng_step_ab.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--curve-rounds", type=int, default=30)
    ap.add_argument("--lr", type=float, default=0.05)
    args = ap.parse_args()
    lines = ["Quantum natural gradient vs SGD-momentum vs Adam on one MI355X (scripts/qng_ab.py)",
             "===================================================================================", "",
             "1. Whole local step, interleaved in one process (median / min ms over the A/B rounds; eager launches,",
             "   8 clients x 32 samples; qng_step = qng_metric_pass + loss_and_grads + qng_step_kernel)", ""]
    for n, L in ((12, 2), (16, 3)):
        lines.append(json.dumps(step_times(n, L, 8, 32, args.rounds, args.iters, args.lr)))
    lines += ["", f"2. {args.curve_rounds} federated rounds on the synthetic 8-qubit task (8 clients x 64 samples, "
                  f"batch 32, 2 layers, lr {args.lr} for all three,",
              "   qng_damping 1e-3): per-round mean local train loss, test loss and test accuracy", ""]
    cv = curves(args.curve_rounds, args.lr)
    for opt, c in cv.items():
        lines.append(json.dumps({"optimizer": opt, **c}))
    lines += ["", "final round: " + ", ".join(f"{o}: train {c['train_loss'][-1]:.4f} test {c['test_loss'][-1]:.4f} "
                                              f"acc {c['test_acc'][-1]:.4f}" for o, c in cv.items())]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
