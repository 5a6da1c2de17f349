"""Interleaved A/B of the MFMA engine's plain local step and its record-level DP-SGD step (csrc/hea_dpsgd.hip) in ONE
process, a sibling of scripts/hea_ab.py.  Each round times, back to back on the same program and inputs: the plain step
(forward, readout, adjoint, hea_grad_reduce; no fused Adam on either side), the DP step (the same passes with the
hea_readout_rec route, then hea_dp_norm + hea_dp_reduce), and the three reductions alone on the slab the step left.
Prints per-item median / min ms over the rounds as JSON.

python scripts/dpsgd_ab.py [--qubits 16 --layers 3 --clients 64 --batch 32 --rounds 7 --iters 10 --sigma 1.0]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("QFX_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=16)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--storage", default="fp16")
    args = ap.parse_args()
    import torch
    from qfedx_amd.models.vqc import VQCSpec
    from qfedx_amd.ops._ext import ext
    from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
    from qfedx_amd.utils.seeding import philox_key

    dev = torch.device("cuda", 0)
    spec = VQCSpec(args.qubits, args.layers, 3)
    K, B = args.clients, args.batch
    S = K * B
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(K, B, args.qubits, generator=g) * 3).to(dev)
    y = torch.randint(0, 3, (K, B), generator=g).to(dev)
    w = torch.full((K, B), 1.0 / B, device=dev)
    ones = torch.ones(K, B, device=dev)
    params = torch.stack([spec.init_params(k) for k in range(K)]).to(dev)
    keys = torch.tensor([philox_key(1, "dpsgd_noise", 0, k) for k in range(K)], dtype=torch.int64, device=dev)
    prog = HeaMfmaProgram(spec, dev, storage=args.storage)
    E = ext()
    dp = dict(clip=1.0, sigma=args.sigma, keys=keys, step=0, lot=B)
    for _ in range(2):
        prog.loss_and_grads(x, y, w, params, spec)
        out = prog.loss_and_grads(x, y, ones, params, spec, dpsgd=dp)
    torch.cuda.synchronize()
    gslab = prog._ws["gslab"][: S * prog.slab_tiles * prog.n_gradops * 32]
    rec = prog._ws["rorec"][: S * (2 * prog.C + 2)]
    grad, loss, correct = torch.empty_like(params), torch.empty(K, device=dev), torch.empty(K, device=dev)
    norm, cfac = torch.empty(S, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev)
    lv = ones.reshape(S).contiguous()
    items = {
        "plain_step": lambda: prog.loss_and_grads(x, y, w, params, spec),
        "dp_step": lambda: prog.loss_and_grads(x, y, ones, params, spec, dpsgd=dp),
        "hea_grad_reduce": lambda: E.hea_grad_reduce(gslab, prog.slab_tiles, prog.n_gradops, prog.gmeta, B, K, params, grad,
                                                     params.shape[1], None, None, [rec, loss, correct], prog.C,
                                                     prog.n_theta),
        "hea_dp_norm": lambda: E.hea_dp_norm(gslab, prog.slab_tiles, prog.n_gradops, prog.gmeta, B, K, params, rec, prog.C,
                                             prog.n_theta, 1.0, norm, cfac),
        "hea_dp_reduce": lambda: E.hea_dp_reduce(gslab, prog.slab_tiles, prog.n_gradops, prog.gmeta, B, K, params, rec, lv,
                                                 cfac, prog.C, prog.n_theta, keys, 0, args.sigma, 1.0, float(B), grad,
                                                 loss, correct),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters

    res = {k: [] for k in items}
    for _ in range(args.rounds):
        for name, fn in items.items():
            res[name].append(timed(fn))
    out = {"qubits": args.qubits, "layers": args.layers, "clients": K, "batch": B, "rounds": args.rounds,
           "iters": args.iters, "sigma": args.sigma, "storage": args.storage,
           "slab_mb": round(gslab.numel() * 8 / 2 ** 20, 1), "readout_mode_plain": prog.readout_mode(S)}
    for name, v in res.items():
        out[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                     "spread_ms": round(max(v) - min(v), 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
