"""Measured errors of the two MPS kernels at their shape edges (profiles/mps_edges_err_table.txt).

    python tools/mps_err_table.py > profiles/mps_edges_err_table.txt      (needs the GPU)

Runs the cases of tests/mps_cases.py exactly as tests/test_gpu_mps_edges.py does and prints, per case and output, the
maximum error of the kernel against the float64 reference, next to it - as the yardstick - the error of the complex64
dense statevector executor on the same float32 inputs, and the bound."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import mps_cases as mc                                                   # noqa: E402
from tests.test_gpu_mps_edges import chain_errors, fused_errors, mpo_errors       # noqa: E402

HEAD = """MPS chain and MPO kernels at their shape edges: error against float64
======================================================================

tests/test_gpu_mps_edges.py on one MI355X.  max |error| over all samples of a case against the float64 reference (the
column oracle for the chain kernel, the complex128 dense statevector for the MPO kernel) on the same float32 inputs;
"dense c64" is the complex64 dense statevector executor on the CPU against the same reference: the yardstick, which
tests/test_mps_cases.py holds under half of the bound.  z = <Z> of the readout launch, z_grad = <Z> of the gradient
launch, grad = per-client gradient sums, dang = per-gate angle derivatives, dl = dL/dlogit, loss / lossv = per-client
/ per-sample loss (bound rtol 1e-4 + atol 1e-5; the column shows the absolute error).  Hits are exact in every case.
"""


def _rows(kernel: str, name: str, shape: str, err: dict, yard: dict, keys: dict) -> None:
    for k, (e, ok, bound) in err.items():
        ref_key, bkey = keys[k]
        y, y_ok = mc.within(bkey, yard[ref_key][0], yard[ref_key][1], 0.5)
        b = f"{bound:.0e}" if isinstance(bound, float) else "rtol"
        print(f"{kernel:<6} {name:<26} {shape:<14} {k:<7} {e:>10.3e} {y:>10.3e} {b:>6}")
        assert ok and y_ok, (name, k, e, y)


def main() -> None:
    print(HEAD)
    print(f"{'kernel':<6} {'case':<26} {'shape':<14} {'output':<7} {'kernel':>10} {'dense c64':>10} {'bound':>6}")
    for c in mc.CHAIN_CASES:
        ref, c64 = mc.chain_reference(c.name), mc.chain_dense(c.name, torch.complex64)
        yard = {k: (c64[k], ref[k]) for k in ("z", "grad")}
        _rows("chain", c.name, f"K{c.K} B{c.B} C{c.C}", chain_errors(c.name), yard,
              dict(z=("z", "z"), z_grad=("z", "z"), grad=("grad", "grad")))
    for c in mc.FUSED_CASES:
        ref, c64 = mc.fused_reference(c.name), mc.chain_dense(c.name, torch.complex64)
        yard = {k: (c64[k], ref[k]) for k in mc.FUSED_KEYS}
        _rows("fused", c.name, f"K{c.K} B{c.B} C{c.C}", fused_errors(c.name), yard,
              {k: (k, b) for k, b in mc.FUSED_KEYS.items()})
    for c in mc.MPO_CASES:
        ref, c64 = mc.mpo_reference(c.name), mc.mpo_dense32(c.name)
        yard = {k: (c64[k], ref[k]) for k in ("z", "dang")}
        _rows("mpo", c.name, f"S{c.S} C{len(c.readout)}",
              mpo_errors(c.name), yard, dict(z=("z", "z"), z_grad=("z", "z"), dang=("dang", "dang")))


if __name__ == "__main__":
    main()
