"""Measured errors of the quantum-natural-gradient kernels against the float64 oracle (profiles/qng_err_table.txt).

    python tools/qng_err_table.py [profiles/qng_err_table.txt]      (needs the GPU)

Runs the cases of tests/qng_cases.py exactly as tests/test_gpu_qng.py does and prints, per case, the maximum error of
the correlator kernel, the engine's metric pass, the step kernel and one federated round.  The last block is the
``MEASURED`` table of tests/qng_cases.py: a test's bound is 3 x its figure."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import qng_cases as qc                                                   # noqa: E402
from tests.test_gpu_qng import corr_errors, metric_errors, round_errors, step_errors   # noqa: E402

HEAD = """Quantum natural gradient on one MI355X: max |kernel - float64 oracle| per case
==================================================================================

tests/test_gpu_qng.py.  The oracle is ops/qng.py in float64 on the CPU from the same float32 / complex64 inputs.
corr:   csrc/qng.hip qng_corr on random normalised complex64 states [S, 2^n] (S = 3; 2 at n = 16): <Z_i>, <Z_i Z_j>.
metric: VQCEngine.metric_blocks on HIP (fp32 VALU pass kernels + qng_corr + qng_blocks), K = 2 clients x B = 3 samples,
        one dead sample, one client without a live sample: the clients' blocks and every sample's blocks.
step:   csrc/qng.hip qng_step against qng_step_ref, K = 3, B = 4, L = 2, lr 0.05, damping 1e-3, one inactive row, one
        exactly-zero block: the updated float32 parameters and the blocks the kernel forms (qng_blocks).
round:  one federated round (4 clients x 48 samples, batch 16, 8 qubits x 2 layers, train.optimizer=qng) on
        runtime.backend=hip against runtime.backend=torch: the global parameters after the round.
"""


def main() -> None:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "qng_err_table.txt")
    lines = []

    def print(text=""):                     # the table goes to the file (run logs share stdout), and to stdout
        lines.append(text)
        sys.stdout.write(text + "\n")

    print(HEAD)
    table = {}
    print(f"{'case':<28} {'quantity':<12} {'max error':>12}")
    for n in qc.CORR_N:
        for k, v in corr_errors(n).items():
            table[f"corr_{n}_{k}"] = v
            print(f"{'corr n=' + str(n):<28} {k:<12} {v:>12.3e}")
    for name, *_ in qc.METRIC_CASES:
        for k, v in metric_errors(name).items():
            table[f"metric_{name}_{k}"] = v
            print(f"{'metric ' + name:<28} {k:<12} {v:>12.3e}")
    for n in qc.STEP_N:
        for k, v in step_errors(n).items():
            table[f"step_{n}_{k}"] = v
            print(f"{'step n=' + str(n):<28} {k:<12} {v:>12.3e}")
    for dt in ("fp32", "mfma"):
        for k, v in round_errors(dt).items():
            table[f"round_{dt}_{k}"] = v
            print(f"{'round state_dtype=' + dt:<28} {k:<12} {v:>12.3e}")
    print("\nMEASURED = {")
    for k, v in table.items():
        print(f'    "{k}": {v:.3e},')
    print("}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
