"""Digests of what the MFMA engine's generating forward pass (pass 0: the layer-1 product state) and the step built
on it compute, for the shapes that reach every branch of the generation block.

python tools/hea_gen_digests.py [--out tests/golden/hea_gen_parent_digests.json]

Run ONCE on the GPU at the commit BEFORE the generation block's fp32 products were pinned in the source (the
interpreter, ``use_spec=False``): the file it writes is what tests/test_gpu_hea_spec_gen.py holds both the interpreter and
the per-plan kernel of pass 0 to, bit for bit.  Uses nothing newer than ``HeaMfmaProgram(spec, dev, tile_bits=,
storage=, use_spec=)`` and ``loss_and_grads``; the tests import the cases and the step from here, so the digests and
the tests cannot drift apart.

Per case: sha256 (first 16 hex digits) of the stored pass-0 state, of <Z>, and of loss + gradient.
"""
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "hea_gen_parent_digests.json")

K, B = 2, 3
# name: (qubits, layers, forward tile bits, storage, feature map, inputs)
#   8q x 1L      one pass, every qubit in the tile, 2^8 amplitudes under 512 threads: quads past the tile read quad 0
#                (wrapped table reads) and store nothing (predicated stores); both half tables hold 4 factors
#   10q x 2L t8  2^8 tiles: two qubits outside the tile (the wave product and outer_s), four tiles per sample
#   16q x 3L     the headline plan: strided window, 7 / 7 table split;  t13: the same plan retiled, 6 / 7
#   inputs       random angles | zero: all-zero features AND parameters (signed zeros through pack_h2) | pi: x = pi
CASES = {
    "8q1L_ry": (8, 1, None, "fp16", "ry", "random"),
    "8q1L_rx_zero": (8, 1, None, "fp16", "rx", "zero"),
    "8q1L_rz_pi": (8, 1, None, "fp16", "rz", "pi"),
    "10q2L_t8_ry": (10, 2, 8, "fp16", "ry", "random"),
    "10q2L_t8_rx_bf16": (10, 2, 8, "bf16", "rx", "random"),
    "10q2L_t8_rz": (10, 2, 8, "fp16", "rz", "random"),
    "16q3L_ry": (16, 3, None, "fp16", "ry", "random"),
    "16q3L_ry_bf16": (16, 3, None, "bf16", "ry", "random"),
    "16q3L_rx_zero": (16, 3, None, "fp16", "rx", "zero"),
    "16q3L_t13_ry": (16, 3, 13, "fp16", "ry", "random"),
    "16q3L_t13_rz_pi": (16, 3, 13, "fp16", "rz", "pi"),
}


def case_spec(name):
    from qfedx_amd.models.vqc import VQCSpec
    n, L, _, _, fm, _ = CASES[name]
    return VQCSpec(n_qubits=n, n_layers=L, n_classes=3, feature_map=fm)


def case_inputs(name, dev):
    """(angles [K, B, n], labels, loss weights, parameters [K, P]) of a case, the same on every machine."""
    import torch
    spec = case_spec(name)
    n, kind = spec.n_qubits, CASES[name][5]
    g = torch.Generator().manual_seed(17)
    xang = spec.encode_features(torch.rand(K, B, n, generator=g))
    y = torch.randint(0, spec.n_classes, (K, B), generator=g)
    w = torch.full((K, B), 1.0 / B)
    params = torch.stack([spec.init_params(k) for k in range(K)])
    params = params + 0.3 * torch.randn(params.shape, generator=g)
    if kind == "zero":
        xang, params = torch.zeros_like(xang), torch.zeros_like(params)
    elif kind == "pi":
        xang = torch.full_like(xang, math.pi)
    return xang.float().to(dev), y.to(dev), w.to(dev), params.float().to(dev)


def run_case(name, dev, **prog_kw):
    """One training step of the case -> (results, program).  Results: ``psi0`` the stored output of forward pass 0 (the
    int32 workspace: packed (re, im) amplitudes), ``expz``, ``loss``, ``grad``."""
    import torch
    from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
    _, _, tile, storage, _, _ = CASES[name]
    spec = case_spec(name)
    xang, y, w, params = case_inputs(name, dev)
    prog = HeaMfmaProgram(spec, dev, tile_bits=tile, storage=storage, **prog_kw)
    out = prog.loss_and_grads(xang, y, w, params, spec)
    torch.cuda.synchronize()
    res = {k: out[k].clone() for k in ("expz", "loss", "grad")}
    res["psi0"] = prog._ws["psi0"][: (K * B) << spec.n_qubits].clone()
    return res, prog


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def digests(res):
    return {"psi0": _sha(res["psi0"]), "expz": _sha(res["expz"]), "loss_grad": _sha(res["loss"], res["grad"])}


def main():
    sys.path.insert(0, os.environ.get("QFX_PKG_ROOT") or ROOT)
    import torch
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    dev = torch.device("cuda", 0)
    table = {}
    for name in CASES:
        res, prog = run_case(name, dev, use_spec=False)
        assert prog.interp_launches > 0 and prog.spec_launches == 0
        assert torch.isfinite(res["grad"]).all() and torch.isfinite(res["expz"]).all()
        table[name] = digests(res)
        print(name, table[name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
