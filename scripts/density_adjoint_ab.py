"""Interleaved A/B of the density simulator's two gradient routes in ONE process -> profiles/density_adjoint_ab.txt:
the reverse sweep (``grad_method=adjoint``: csrc/density_adj.hip) against the parameter-shift route
(``grad_method=param_shift``: 2 n_theta + 1 evolutions per sample through csrc/density.hip), the same engine, inputs
and parameters.  Per shape it runs ``--repeats`` rounds of (adjoint steps, shift steps), each timed with device
events around ``--iters`` steps after one untimed step, and records the step times, the tape size, and per step the
circuit evolutions (rows through the kernels) and kernel launches of each route.

python scripts/density_adjoint_ab.py [--out FILE] [--shapes 4x2,8x3 --clients 8 --batch 16 --gamma 0.05 --repeats 3]
"""
import argparse
import json
import os
import sys

ROOT = os.environ.get("QFX_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x2,8x3")
    ap.add_argument("--clients", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--gamma", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_adjoint_ab.txt"))
    args = ap.parse_args()
    import torch
    from qfedx_amd.models.vqc import VQCSpec
    from qfedx_amd.ops._ext import ext
    from qfedx_amd.ops.engine import VQCEngine
    from qfedx_amd.quantum.noise import NoiseModel

    if not torch.cuda.is_available():
        raise SystemExit("scripts/density_adjoint_ab.py times GPU kernels: no GPU visible")
    dev = torch.device("cuda", 0)
    E = ext()
    count = {"launches": 0, "rows": 0}
    for name in ("dm_run", "dm_forward_tape", "dm_adjoint"):
        def wrapped(*a, _fn=getattr(E, name), _fwd=name != "dm_adjoint"):
            count["launches"] += 1
            count["rows"] += a[3].shape[0] if _fwd else 0         # rows evolved forward (the backward sweep: none)
            return _fn(*a)
        setattr(E, name, wrapped)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    K, B = args.clients, args.batch
    lines = ["Density simulator, one local step: reverse sweep (adjoint) against parameter shift, interleaved in one process",
             f"one MI355X; {K} clients x {B} samples, noise.kind=amplitude gamma={args.gamma}; {args.repeats} repeats of "
             f"(adjoint, shift), {args.iters} timed steps each after one untimed; ms per step", ""]
    results = []
    for shape in args.shapes.split(","):
        n, L = (int(v) for v in shape.split("x"))
        spec = VQCSpec(n, L, 3, readout_scale=2.0)
        eng = VQCEngine(spec, dev, "density", noise=NoiseModel(kind="amplitude", gamma=args.gamma))
        g = torch.Generator().manual_seed(n)
        x = spec.encode_features(torch.rand(K, B, n, generator=g)).to(dev)
        y = torch.randint(0, 3, (K, B), generator=g).to(dev)
        w = torch.full((K, B), 1.0 / B, device=dev)
        params = torch.stack([spec.init_params(k) for k in range(K)]).to(dev)
        steps = {m: (lambda m=m: eng.loss_and_grads(x, y, w, params, m)) for m in ("adjoint", "param_shift")}
        per_step, grads = {}, {}
        for m, fn in steps.items():                                # warm-up, counted
            fn()
            count["launches"] = count["rows"] = 0
            grads[m] = fn()["grad"]
            per_step[m] = dict(count)
        torch.cuda.synchronize()
        times = {m: [] for m in steps}
        for _ in range(args.repeats):
            for m, fn in steps.items():
                times[m].append(timed(fn))
        ratio = min(times["param_shift"]) / max(times["adjoint"])
        rec = {"qubits": n, "layers": L, "n_theta": spec.n_theta, "clients": K, "batch": B,
               "path": "LDS" if n <= E.dm_lds_qubits() else "global slab",
               "tape_bytes_per_sample": eng.prog.tape_bytes(spec.n_theta),
               "tape_bytes_per_step": eng.prog.tape_bytes(spec.n_theta) * K * B,
               "adjoint_ms": [round(t, 4) for t in times["adjoint"]],
               "param_shift_ms": [round(t, 4) for t in times["param_shift"]],
               "adjoint": per_step["adjoint"], "param_shift": per_step["param_shift"],
               "every_adjoint_run_faster": max(times["adjoint"]) < min(times["param_shift"]),
               "slowest_adjoint_over_fastest_shift_speedup": round(ratio, 2),
               "max_grad_diff": float((grads["adjoint"] - grads["param_shift"]).abs().max())}
        results.append(rec)
        lines += [f"{n}q x {L}L ({rec['path']}; n_theta = {spec.n_theta}; tape {rec['tape_bytes_per_sample']} B per sample, "
                  f"{rec['tape_bytes_per_step'] / 2 ** 20:.2f} MiB per step)",
                  f"  adjoint      ms {rec['adjoint_ms']}   evolutions {per_step['adjoint']['rows']:>6}  launches "
                  f"{per_step['adjoint']['launches']}",
                  f"  param_shift  ms {rec['param_shift_ms']}   evolutions {per_step['param_shift']['rows']:>6}  launches "
                  f"{per_step['param_shift']['launches']}",
                  f"  every adjoint run faster than every shift run: {rec['every_adjoint_run_faster']}; fastest shift / "
                  f"slowest adjoint = {ratio:.2f}x; max |grad difference| {rec['max_grad_diff']:.2e}", ""]
    text = "\n".join(lines) + "\n".join(json.dumps(r) for r in results) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
