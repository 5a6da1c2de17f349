"""CPU twin of tests/test_gpu_mps_edges.py: what the cases of tests/mps_cases.py reach and what their references are.

* MPO cases: the MPS that the compiled event tables define (the torch emulator ``site_tensors``) equals the complex128
  dense statevector, and the coverage the case table claims - four pass-throughs on a site, a 16-wide bond on two
  qubits, a product cut inside a chain, an idle qubit, 64 rotations on one qubit, every (event type, side, bond bit)
  combination, every 1-qubit kind, every fixed kind between two rotations behind an entangler - is asserted from the
  tables.
* Chain cases: the column oracle ``chain_columns`` equals the complex128 dense statevector at n = 2, n = 3, C = 8,
  repeated readout qubits and angles in [-7, 7]; the fused reference has a clear argmax on every sample.
* Input conditions: on every case the complex64 dense executor stays within half of the GPU bound of float64 and the
  reference gradient is not degenerate, so a GPU case over its bound is a finding about the kernel."""
import numpy as np
import pytest
import torch

from qfedx_amd.ops.statevec_torch import PAULI
from qfedx_amd.quantum.mps import MPS
from qfedx_amd.quantum.mps_mpo import EV_CTRL, EV_GATE, EV_X, EV_Z, ROTATIONS, compile_mpo, site_tensors
from tests import mps_cases as mc

MPO_IDS = [c.name for c in mc.MPO_CASES]
CHAIN_IDS = [c.name for c in mc.CHAIN_CASES]
FUSED_IDS = [c.name for c in mc.FUSED_CASES]
FIXED_KINDS = set(range(4, 13))


def _err(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref).abs().max())


# ------------------------------------------------------------------------------------------------ MPO tables
@pytest.mark.parametrize("name", MPO_IDS)
def test_mpo_tables_define_the_dense_state(name):
    ang = mc.mpo_inputs(name)["ang"].double()
    st = MPS(site_tensors(mc.mpo_tables(name), ang))
    np.testing.assert_allclose(st.to_dense().numpy(), mc.mpo_reference(name)["psi"].numpy(), atol=1e-12)


def test_mpo_cases_reach_the_table_edges():
    tabs = {n: mc.mpo_tables(n) for n in MPO_IDS}
    nbits = {n: t["nbits"].tolist() for n, t in tabs.items()}
    sinfo = {n: t["sinfo"].tolist() for n, t in tabs.items()}
    assert nbits["passover4"] == [0, 4, 4, 4, 4]
    assert [r[3] for r in sinfo["passover4"]] == [0, 0, 4, 4, 4, 0]
    for n in ("two_qubits_d16", "two_qubits_d16_s1", "two_qubits_d16_s2", "two_qubits_d16_s3"):
        assert nbits[n] == [4]
    assert nbits["uneven_bonds"] == [1, 4, 2, 0, 3]                     # a 0-bit cut strictly inside, Dl != Dr
    assert nbits["swap3"] == [3, 3] and sinfo["swap3"][1][3] == 3
    assert nbits["ring4"] == [4, 4, 4]
    assert [r[1] for r in sinfo["idle_qubits"]] == [0, 6, 0, 6, 0]      # cnt == 0 at both ends and under a pass-over
    assert sinfo["idle_qubits"][2][3] == 2
    assert sinfo["maxpg64"][1][4] == 64
    assert any(0 in b[1:-1] for b in nbits.values())


def test_mpo_cases_cover_every_event_and_kind():
    events = [ev for n in MPO_IDS for site in mc.mpo_events(n) for ev in site]
    combos = {(t, side, bit) for t, side, bit, _ in events if t != EV_GATE}
    assert combos == {(t, side, bit) for t in (EV_CTRL, EV_X, EV_Z) for side in (0, 1) for bit in range(4)}
    kinds = {k for t, _, _, k in events if t == EV_GATE}
    assert kinds == set(range(13)) | {PAULI}
    ro = [c.readout for c in mc.MPO_CASES]
    assert any(len(r) == 1 for r in ro) and any(len(r) == 8 and len(set(r)) < 8 for r in ro)
    assert any(max(r) == 0 for r in ro) and {c.S for c in mc.MPO_CASES} == {1, 5}
    assert any(max(c.readout) < c.n - 2 for c in mc.MPO_CASES) and any(c.n - 1 in c.readout for c in mc.MPO_CASES)


def _between_rotations(site, wanted) -> set:
    """Kinds of ``wanted`` that sit directly between two rotations behind a CX / CZ event of this site."""
    found, entangled = set(), False
    for i, (t, _, _, k) in enumerate(site):
        entangled |= t != EV_GATE
        if t == EV_GATE and k in wanted and entangled and 0 < i < len(site) - 1:
            (tp, _, _, kp), (tn, _, _, kn) = site[i - 1], site[i + 1]
            if tp == EV_GATE and tn == EV_GATE and kp in ROTATIONS and kn in ROTATIONS:
                found.add(k)
    return found


def test_fixed_gates_and_paulis_sit_between_rotations():
    sites = mc.mpo_events("fixed_between_rotations")
    assert set().union(*(_between_rotations(s, FIXED_KINDS) for s in sites)) == FIXED_KINDS
    assert any(k == 3 for s in sites for t, _, _, k in s if t == EV_GATE)            # P among the rotations
    for s in sites:
        assert any(t != EV_GATE for t, _, _, _ in s)                                 # every qubit carries a CX / CZ end
    for s in mc.mpo_events("pauli_selectors"):
        assert _between_rotations(s, {PAULI}) == {PAULI}
    i = mc.mpo_inputs("pauli_selectors")
    sel = i["ang"][:, mc.mpo_tables("pauli_selectors")["gkind"] == PAULI]
    for col in sel.T:
        assert set(col.tolist()) == {0.0, 1.0, 2.0, 3.0}


def test_maxpg64_every_rotation_has_a_derivative():
    d = mc.mpo_reference("maxpg64")["dang"].abs()
    mask = mc.mpo_inputs("maxpg64")["mask"]
    assert int(mask.sum()) == 69
    assert float(d[:, mask].min()) > 1e-5                  # nonzero in every sample
    assert float(d[:, mask].max(0).values.min()) > 1e-2    # and far above the 5e-5 bound in some sample


def test_over_wide_programs_are_refused():
    with pytest.raises(ValueError, match="more than 64 rotations"):
        compile_mpo(mc.ops_list(mc.maxpg64(extra=1)[0]), 3)
    with pytest.raises(ValueError, match="bond > 16"):
        compile_mpo(mc.ops_list(mc.five_on_a_cut()[0]), 2)


@pytest.mark.parametrize("name", MPO_IDS)
def test_mpo_input_conditions(name):
    ref, c64 = mc.mpo_reference(name), mc.mpo_dense32(name)
    assert _err(c64["z"], ref["z"]) < 0.5 * mc.TOL["z"]
    assert _err(c64["dang"], ref["dang"]) < 0.5 * mc.TOL["dang"]
    assert float(ref["dang"].abs().max()) > 1e-2
    if name == "idle_qubits":                              # <Z> = 1 on the idle qubits 0, 2, 4
        assert float((ref["z"][:, [0, 2, 3]] - 1).abs().max()) < 1e-14


def test_simulator_case_shares_a_parameter_and_has_a_constant_rotation():
    ops, coef = mc.shared_parameter_circuit().to_program({"v": 0})
    rows = [(k, q, s, float(a)) for (k, q, _, s), (a, _) in zip(ops.tolist(), coef.tolist()) if k in ROTATIONS]
    for slot in range(4):
        uses = [(q, a) for _, q, s, a in rows if s == slot]
        assert len(uses) == 2 and uses[0][0] != uses[1][0]
    assert len({a for _, _, s, a in rows if s == 0}) == 2          # different coefficients
    assert sum(s == -1 for _, _, s, _ in rows) == 2                # constant-angle rotations
    compile_mpo(mc.ops_list(ops), 4)


# ------------------------------------------------------------------------------------------------ chain oracle
@pytest.mark.parametrize("name", CHAIN_IDS)
def test_chain_oracle_matches_dense_and_input_conditions(name):
    ref, c128, c64 = mc.chain_reference(name), mc.chain_dense(name), mc.chain_dense(name, torch.complex64)
    assert _err(c128["z"], ref["z"]) < 1e-10
    assert _err(c128["grad_s"], ref["grad_s"]) < 1e-10
    assert _err(c64["z"], ref["z"]) < 0.5 * mc.TOL["z"]
    assert _err(c64["grad"], ref["grad"]) < 0.5 * mc.TOL["grad"]
    assert float(ref["grad"].abs().max()) > 1e-2


@pytest.mark.parametrize("name", FUSED_IDS)
def test_fused_reference(name):
    ref, c128, c64 = mc.fused_reference(name), mc.chain_dense(name), mc.chain_dense(name, torch.complex64)
    i = mc.chain_inputs(name)
    for key in ("z", "loss", "grad", "dl", "lossv"):
        assert _err(c128[key], ref[key]) < 1e-10, key
    for key, bound in mc.FUSED_KEYS.items():
        e, ok = mc.within(bound, c64[key], ref[key], 0.5)
        assert ok, (key, e)
    assert torch.equal(c64["hitv"].double(), ref["hitv"]) and torch.equal(c128["correct"], ref["correct"])
    lg = ref["logits"].sort(-1).values
    assert float((lg[:, -1] - lg[:, -2]).min()) > mc.LOGIT_GAP           # every sample, weighted or not
    wm, a = i["wmask"], i["params"][:, -2 * len(mc.CHAIN_BY_NAME[name].readout):-len(mc.CHAIN_BY_NAME[name].readout)]
    assert int((wm == 0).sum()) == 2 and len(set(wm[wm > 0].tolist())) == 7
    assert bool((a > 0).any(1).all()) and bool((a < 0).any(1).all()) and bool((i["params"][:, -1] != 0).all())
    assert 0 < float(ref["hitv"].sum()) < float((wm > 0).sum())            # hits and misses both occur
    assert float(ref["grad"].abs().max()) > 1e-2


def test_chain_case_table_covers_the_issue():
    by = {(c.n, c.L, c.feature) for c in mc.CHAIN_CASES}
    assert {(4, L, f) for L in (1, 2, 3) for f in ("ry", "rx", "rz")} <= by
    for stem in ("n2_L3_c8", "n10_L3_rz_c8", "n10_L2_rx_ro210"):
        assert {(c.K, c.B) for c in mc.CHAIN_CASES if c.name.startswith(stem)} == set(mc.BATCHES)
    assert {c.variant for c in mc.CHAIN_CASES} == {"", "rows", "xpad"}
    i = mc.chain_inputs("n3_L3_ry_xpad")
    assert i["xarg"].shape[-1] == 6 and bool(i["xarg"][..., 3:].isnan().all())
    assert mc.chain_inputs("n10_L2_rx_rows")["targ"].shape[1] == 40 + 6
