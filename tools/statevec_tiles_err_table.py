"""Measured errors of the generic statevector kernels at every tile shape (profiles/statevec_tiles_err_table.txt).

    python tools/statevec_tiles_err_table.py > profiles/statevec_tiles_err_table.txt      (needs the GPU)

Runs the cases of tests/statevec_cases.py exactly as tests/test_gpu_statevec_tiles.py does and prints, per case and
start (product state / complex initial states / raw real rows), the maximum error of the interpreter kernel, the
per-plan kernels and - as the yardstick - the fp32 torch executor against the same float64 reference."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import statevec_cases as sc                      # noqa: E402
from tests.test_gpu_statevec_tiles import TOL, errors      # noqa: E402

HEAD = """Generic (VALU) statevector kernels at every tile shape: error against the float64 torch executor
=========================================================================================================

tests/test_gpu_statevec_tiles.py on one MI355X, K = 3 parameter rows x B = 3 samples, HipProgram(kmax=) forcing the
tile; T = threads per tile.  max |d amplitude|, max |d<Z>| (the worst of the train plan, the evaluation plan and the
vjp's forward) and max |d grad| over all samples / parameter rows, per start: prod = product state, cplx = complex
initial states, real = raw real rows encoded on device.  "torch32" is the fp32 torch executor on the CPU against the
same reference: the yardstick.  "x" = worst ratio kernel / yardstick of the row's three columns.
Bounds (tests/test_gpu_simulator.py, against float64): 2e-5 amplitudes and <Z>, 5e-5 gradients.
"""


def main() -> None:
    print(HEAD)
    print(f"{'case':<16} {'n':>2} {'k':>2} {'T':>3} {'kernel':<7} {'start':<5} {'amplitude':>10} {'<Z>':>10} "
          f"{'grad':>10} {'x':>6}")
    worst = 0.0
    for c in sc.CASES:
        T = 1 << (c.kmax - (c.R.bit_length() - 1))
        yard = sc.executor_errors(c.name)
        runs = [("interp", errors(c.name, False))] + ([("jit", errors(c.name, True))] if c.jit else [])
        for start in ("prod", "cplx", "real"):
            y = yard[start]
            print(f"{c.name:<16} {c.n:>2} {c.kmax:>2} {T:>3} {'torch32':<7} {start:<5} {y['psi']:>10.3e} "
                  f"{y['z']:>10.3e} {y['grad']:>10.3e}")
            for kern, err in runs:
                e = err[start]
                z = max(e["z"], e["z_vjp"], e.get("z_eval", 0.0))
                ratio = max(e["psi"] / y["psi"], z / y["z"], e["grad"] / y["grad"])
                worst = max(worst, ratio)
                print(f"{'':<16} {'':>2} {'':>2} {'':>3} {kern:<7} {start:<5} {e['psi']:>10.3e} {z:>10.3e} "
                      f"{e['grad']:>10.3e} {ratio:>6.1f}")
                assert e["psi"] < TOL["psi"] and z < TOL["z"] and e["grad"] < TOL["grad"]
    print(f"\nworst kernel / yardstick ratio: {worst:.1f}")


if __name__ == "__main__":
    main()
