"""Measured errors of the density simulator's reverse sweep -> profiles/density_adjoint_err_table.txt.

    python tools/density_adjoint_err_table.py [--out FILE]      (needs the GPU)

Runs the cases of tests/density_adjoint_cases.py exactly as tests/test_gpu_density_adjoint.py does and records, per
case, max |d<Z>| and max |d grad| of the tape forward + backward kernels (csrc/density_adj.hip) against the float64
shift-rule oracle, and - as the yardstick - the same two errors of the fp32 parameter-shift route through the forward
kernel (csrc/density.hip) on the same inputs.  The test bounds are 3 x the "adjoint" columns."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                                            # noqa: E402

from tests.density_adjoint_cases import GPU_CASES                      # noqa: E402
from tests.test_gpu_density_adjoint import TOL, errors, shift_errors   # noqa: E402

HEAD = """Density-matrix reverse sweep (csrc/density_adj.hip): error against the float64 shift-rule oracle
=====================================================================================================

tests/test_gpu_density_adjoint.py on one MI355X, S = 3 rows per case, w ~ N(0, 1) per readout qubit.  "adjoint" = the
tape forward + backward kernels; "shift" = the fp32 parameter-shift route through the forward kernel (every
differentiated gate at +-pi/2, pair differences accumulated in float64): existing code, the yardstick.  G = gates,
J = differentiated gates (tape entries per row).  bound = 3 x the adjoint error, the figures in the test's TOL.
"vs shift" = bound over 3 x the shift route's error: above 1, the bound is wider than the yardstick's would be.
"""

NOTE = """
<Z> of the tape forward is bitwise dm_run's, so the two <Z> columns agree.  Where "vs shift" is above 1 (n8_ideal, the
gradient bound) the test bound is wider than 3 x the shift route's error would be.  The reverse sweep forms each
gate's gradient as an fp32 sum over the 4^(n-1) quads (64 terms per thread, then a 256-way tree), the shift route as a
float64 difference of two <Z>, each an fp32 sum over 2^n diagonal entries; n8_ideal is the largest case and, without a
channel, has the largest gradients of the table (|grad| up to 1.6: its error is 6 ulp of that in fp32, the shift
route's 3.5).  The bound stays 3 x the measured error of the new path, as for every other case."""


def main() -> None:
    out = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
           else os.path.join(ROOT, "profiles", "density_adjoint_err_table.txt"))
    if not torch.cuda.is_available():
        raise SystemExit("tools/density_adjoint_err_table.py measures GPU kernels: no GPU visible")
    dev = torch.device("cuda", 0)
    lines = [HEAD, f"{'case':<12} {'n':>2} {'G':>3} {'J':>3} | {'adjoint <Z>':>11} {'grad':>10} | {'shift <Z>':>10} "
                   f"{'grad':>10} | {'bound <Z>':>10} {'grad':>10} {'vs shift':>8} {'in TOL':>6}"]
    for name, make in GPU_CASES.items():
        prog, _, _, n_grad = make("cpu")
        a, s = errors(name, dev), shift_errors(name, dev)
        bz, bg = 3 * a["z"], 3 * a["grad"]
        ratio = max(bz / (3 * s["z"]) if s["z"] > 0 else 1.0, bg / (3 * s["grad"]) if s["grad"] > 0 else 1.0)
        tz, tg = TOL[name]
        held = "-" if tz is None else ("yes" if a["z"] <= tz and a["grad"] <= tg else "NO")
        lines.append(f"{name:<12} {prog.n:>2} {len(prog.ops):>3} {len(prog.taped_gates(n_grad)):>3} | {a['z']:>11.3e} "
                     f"{a['grad']:>10.3e} | {s['z']:>10.3e} {s['grad']:>10.3e} | {bz:>10.3e} {bg:>10.3e} {ratio:>8.2f} "
                     f"{held:>6}")
    lines.append(NOTE)
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
