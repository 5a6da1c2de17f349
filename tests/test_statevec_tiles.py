"""CPU twin of tests/test_gpu_statevec_tiles.py: the plans of every case of tests/statevec_cases.py (tile sizes
k = 2..12, every threads-per-tile count from 1 to 256, qubits outside the tile) run through the register-level float64
emulator of the pass kernels and must reproduce the float64 oracle; and a coverage test proves that the cases - those
that run on the interpreter and, separately, those that also run on the per-plan kernels - reach every micro-op /
bit-class combination the kernels implement.  1e-6 is the bound of the float32 gate tables (tests/test_planner.py)."""
import numpy as np
import pytest
import torch

from qfedx_amd.ops.plan_tools import emulate_adjoint, emulate_forward, emulate_pass, parse_blob
from qfedx_amd.quantum.statevector import Statevector
from tests import statevec_cases as sc

C = pytest.importorskip("qfedx_amd._qfedx_C", reason="native extension not built")

ALL = sc.CASES + [sc.BF16_CASE]
TOL = 1e-6
SAMPLES = (0, 4, 8)            # one sample of each parameter row; sample 4 is the all-zero (-> uniform) raw row


def _plans(case) -> dict:
    ops, coef = case.program()
    return {m: parse_blob(C.plan(torch.from_numpy(ops), torch.from_numpy(coef), case.n, case.R, case.kmax,
                                 list(case.readout), case.n_theta, mode, fin))
            for m, (mode, fin) in sc.MODES.items()}


def _features(case) -> set:
    rb = case.R.bit_length() - 1
    return {f"{m}/{f}" for m, info in _plans(case).items() for f in sc.plan_features(info, rb)}


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_plans_emulated_match_float64(case):
    plans, ref, inp = _plans(case), sc.reference(case.name), sc.inputs(case.name)
    ops, coef = case.program()
    rows = sc.rows_of(case.name).numpy()
    starts = sc.start_states(case.name)
    nt = case.n_theta
    grad_gate = np.array([0 <= s < nt and k <= 3 for k, s in zip(ops[:, 0], ops[:, 3])])
    for s in SAMPLES:
        th, x, w = rows[s, :nt], rows[s, nt:], inp["w"][s].double().numpy()
        psi, z = emulate_forward(plans["fwd"], th, x)
        assert np.abs(psi - ref["prod"]["psi"][s].numpy()).max() < TOL
        assert np.abs(z - ref["prod"]["z"][s].numpy()).max() < TOL
        for start in ("cplx", "real"):                    # load-from-state plan
            psi = starts[start][s].numpy().copy()
            for p in plans["load"]["passes"]:
                z = emulate_pass(plans["load"], p, psi, None, th, x, None, False, None)
            assert np.abs(psi - ref[start]["psi"][s].numpy()).max() < TOL
            assert np.abs(z - ref[start]["z"][s].numpy()).max() < TOL
        for start in ("prod", "cplx"):
            g = emulate_adjoint(plans["adj"], ref[start]["psi"][s].numpy(), th, x, w)
            slot = np.zeros(nt)
            np.add.at(slot, ops[grad_gate, 3], g[grad_gate] * coef[grad_gate, 0])
            assert np.abs(slot - ref[start]["grad_s"][s].numpy()).max() < TOL


@pytest.mark.parametrize("case", [sc.BY_NAME["dir_9q_k6"], sc.BY_NAME["rand_6q_k4"]], ids=lambda c: c.name)
def test_reference_matches_statevector_oracle(case):
    """The shared float64 reference (the torch executor in complex128) against the independent numpy oracle, swap and
    Pauli selectors included."""
    rows = sc.rows_of(case.name).numpy()
    for s in SAMPLES:
        sv = Statevector.from_instruction(case.build(), {"theta": rows[s, :case.n_theta], "x": rows[s, case.n_theta:]})
        assert np.abs(sv.data - sc.reference(case.name)["prod"]["psi"][s].numpy()).max() < TOL
        zs = [sv.expectation_z(q) for q in case.readout]
        assert np.abs(np.array(zs) - sc.reference(case.name)["prod"]["z"][s].numpy()).max() < TOL


def test_grid_tile_shapes():
    """(n, kmax, R) -> threads per tile, tiles per workgroup, tiles per sample of the grid."""
    got = {(c.n, c.kmax): (1 << (c.kmax - (c.R.bit_length() - 1)), 256 >> (c.kmax - (c.R.bit_length() - 1)),
                           1 << (c.n - c.kmax)) for c in sc.CASES}
    assert got == {(3, 2): (1, 256, 2), (6, 4): (1, 256, 4), (7, 5): (2, 128, 4), (9, 6): (4, 64, 8),
                   (10, 7): (8, 32, 8), (11, 8): (16, 16, 8), (11, 10): (64, 4, 2), (12, 10): (64, 4, 4),
                   (13, 11): (128, 2, 4), (14, 12): (256, 1, 4)}
    assert sc.BY_NAME["r4_3q_k2"].R == 4 and all(c.R == 16 for c in sc.CASES[1:])
    assert {c.name for c in sc.CASES if c.jit} == {"rand_6q_k4", "dir_9q_k6", "rand_11q_k10", "dir_12q_k10",
                                                   "rand_13q_k11", "rand_14q_k12"}
    assert len(sc.BY_NAME["dir_9q_k6"].readout) == 8 and len(sc.BY_NAME["dir_12q_k10"].readout) == 1


def test_plan_feature_coverage():
    """Every case reaches what it claims, and the cases of each kernel together reach every required feature."""
    feats = {c.name: _features(c) for c in ALL}
    for c in ALL:
        assert c.features, c.name
        assert not c.features - feats[c.name], (c.name, sorted(c.features - feats[c.name]))
    interp = set().union(*(feats[c.name] for c in sc.CASES))
    jit = set().union(*(feats[c.name] for c in sc.CASES if c.jit))
    assert not sc.REQUIRED - interp, sorted(sc.REQUIRED - interp)
    assert not sc.REQUIRED - jit, sorted(sc.REQUIRED - jit)
    # the fused-group limit: a forward group of MAX_GROUP and its overflow group, on both kernels' directed cases
    for name in ("dir_9q_k6", "dir_12q_k10"):
        assert "fwd/G1:8" in feats[name] and not any(f.startswith("fwd/G1:9") for f in feats[name])
