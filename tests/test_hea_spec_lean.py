"""The lean per-plan kernels (``HeaMfmaProgram.spec_lean`` / ``QFEDX_HEA_SPEC_LEAN``, csrc/hea_spec.h ``HEA_LEAN_*``),
the parts that need no GPU: for five programs the generated prelude marks exactly the expected op boundaries as
barrier-free and the expected passes as early-store, a pass in which no part finds work keeps its text and key, each
part is switched by its own bit, and mask 0 generates the text of before the knob (the shorter configuration list).

The expected marks are read off the op lists (asserted here too, so a planner change shows up as such):

  8q x 2L            adj0  OBS BACK BACK GRAD_L1 GRAD_L1            no barrier before op 4
  11q x 2L           adj0  OBS BACK BACK2 GRAD2 GRAD_L1             no barrier before op 4, held im rows
  13q x 2L           adj0  OBS BACK BACK BACK2 GRAD2 GRAD2          no barrier before op 5, held im rows
  14q x 2L, t 13/13  adj0  BACK BACK2 GRAD2 GRAD2                   no barrier before op 3, held im rows
                     adj1  OBS BACK GRAD_L1 (stores lambda)         lambda stored at op 2's barrier
  16q x 3L           adj0  BACK2 BACK BACK2 GRAD2 GRAD2             no barrier before op 4, held im rows
                     adj1  OBS BACK2 BACK GRAD_L1 (stores lambda)   lambda stored at op 3's barrier, held im rows
  every forward pass that ends in READOUT stores its tile at that op's barrier; the others keep their text.
"""
import re

import pytest

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_mfma
from qfedx_amd.ops import hea_plan as hp
from qfedx_amd.ops._ext import ext
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram, spec_lean_default
from qfedx_amd.ops.statevec_hip import ARCH, CSRC

O, B, B2, G2, G1, A, A2, R = (hp.OP_OBS, hp.OP_BACK, hp.OP_BACK2, hp.OP_GRAD2, hp.OP_GRAD_L1, hp.OP_APPLY, hp.OP_APPLY2,
                              hp.OP_READOUT)
# name: (qubits, layers, forward tile bits), and per pass program its op codes and (mask, barrier-free ops, early op)
# with every part requested; mask 0: the text carries no trace of the knob
CASES = {
    "8q2L": ((8, 2, None), {"fwd0": ([A, A, R], (4, [], 2)), "adj0": ([O, B, B, G1, G1], (2, [4], -1))}),
    "11q2L": ((11, 2, None), {"fwd0": ([A2, A, R], (4, [], 2)), "adj0": ([O, B, B2, G2, G1], (3, [4], -1))}),
    "13q2L": ((13, 2, None), {"fwd0": ([A2, A, A, R], (4, [], 3)), "adj0": ([O, B, B, B2, G2, G2], (3, [5], -1))}),
    "14q2L_t13": ((14, 2, 13), {"fwd0": ([A2, A], (0, [], -1)), "adj0": ([B, B2, G2, G2], (3, [3], -1)),
                                "fwd1": ([A, R], (4, [], 1)), "adj1": ([O, B, G1], (4, [], 2))}),
    "16q3L": ((16, 3, None), {"fwd0": ([A2, A, A2], (0, [], -1)), "adj0": ([B2, B, B2, G2, G2], (3, [4], -1)),
                              "fwd1": ([A, A2, R], (4, [], 2)), "adj1": ([O, B2, B, G1], (5, [], 3))}),
}


@pytest.fixture
def env(monkeypatch):
    for name in ("QFEDX_HEA_SPLIT_RO", "QFEDX_HEA_SPEC", "QFEDX_HEA_SPEC_GEN", "QFEDX_HEA_SPEC_LEAN", "QFEDX_DEBUG",
                 "QFEDX_STAMPS", "QFEDX_HEA_OBS_LOAD", "QFEDX_HEA_TILE", "QFEDX_HEA_ADJ_TILE", "QFEDX_EXTRA_HIPFLAGS"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _program(name, mask, storage="fp16"):
    (n, L, tile), _ = CASES[name]
    return HeaMfmaProgram(VQCSpec(n, L, 3), "cpu", tile_bits=tile, storage=storage, use_spec=False, spec_lean=mask)


def _passes(prog):
    for j, ((f, ff), (a, fa)) in enumerate(prog._host_progs):
        if j <= prog.fwd_last and len(f):
            yield f"fwd{j}", False, j, f, ff
        if len(a):
            yield f"adj{j}", True, j, a, fa


def _marks(text):
    """(mask, barrier-free ops, early-store op) as the prelude text states them."""
    m = re.search(r"^#define QFX_HEA_SPEC_LEAN (\d+)$", text, re.M)
    if not m:
        assert "LEAN" not in text and "NOBAR" not in text and "EARLY_STORE" not in text
        return 0, [], -1
    nobar = [int(v) for v in re.search(r"constexpr int NOBAR\[NOPS\] = \{([^}]*)\};", text).group(1).split(",")]
    early = int(re.search(r"constexpr int EARLY_STORE = (-?\d+);", text).group(1))
    return int(m.group(1)), [o for o, v in enumerate(nobar) if v], early


def test_the_knob_is_read_when_the_program_is_built(env):
    assert hea_mfma.SPEC_LEAN_ENGINE in range(8)
    assert spec_lean_default() == 0 and spec_lean_default(5) == 5              # unset: the caller decides
    direct = HeaMfmaProgram(VQCSpec(8, 2, 3), "cpu", use_spec=False)
    assert direct.spec_lean == 0 and len(direct.spec_cfg(0, True)) == 19       # the list of before the knob
    for value in ("0", "1", "6", "7"):
        env.setenv("QFEDX_HEA_SPEC_LEAN", value)
        assert spec_lean_default(7) == int(value)
        prog = HeaMfmaProgram(VQCSpec(8, 2, 3), "cpu", use_spec=False)
        assert prog.spec_lean == int(value)
        cfg = prog.spec_cfg(0, True)
        assert (len(cfg), cfg[19:]) == ((20, [int(value)]) if int(value) else (19, []))
    assert HeaMfmaProgram(VQCSpec(8, 2, 3), "cpu", use_spec=False, spec_lean=2).spec_lean == 2   # an argument wins
    env.setenv("QFEDX_HEA_SPEC_LEAN", "8")
    with pytest.raises(ValueError):
        spec_lean_default()


def test_engine_asks_for_it(env):
    from qfedx_amd.ops.engine import VQCEngine
    seen = []

    class Recorder:
        def __init__(self, *a, **kw):
            seen.append(kw)

    env.setattr(hea_mfma, "HeaMfmaProgram", Recorder)
    VQCEngine(VQCSpec(n_qubits=8, n_layers=1, n_classes=3), "cpu", "hip", "mfma")
    env.setenv("QFEDX_HEA_SPEC_LEAN", "0")
    VQCEngine(VQCSpec(n_qubits=8, n_layers=1, n_classes=3), "cpu", "hip", "mfma_bf16")
    assert [kw["spec_lean"] for kw in seen] == [hea_mfma.SPEC_LEAN_ENGINE, 0]


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_prelude_marks_the_expected_boundaries_and_stores(env, name, storage):
    C = ext()
    prog = _program(name, 7, storage)
    want = CASES[name][1]
    seen = {}
    for pname, adjoint, j, ops, fidx in _passes(prog):
        assert [int(w[hp.W_CODE]) for w in ops] == want[pname][0], pname
        seen[pname] = _marks(C.hea_spec_source(adjoint, ops, fidx, prog.spec_cfg(j, adjoint)))
    assert seen == {k: v[1] for k, v in want.items()}
    # a region ring keeps every barrier (its flush runs behind them): none here, as the marks above need
    assert all(nr <= 9 for nr in prog.n_regions)


@pytest.mark.parametrize("name", list(CASES))
def test_each_part_has_its_own_bit(env, name):
    C = ext()
    full = CASES[name][1]
    for bit in (1, 2, 4):
        prog = _program(name, bit)
        for pname, adjoint, j, ops, fidx in _passes(prog):
            mask, nobar, early = full[pname][1]
            got = _marks(C.hea_spec_source(adjoint, ops, fidx, prog.spec_cfg(j, adjoint)))
            if mask & bit:
                assert got == (bit, nobar if bit == 2 else [], early if bit == 4 else -1), (pname, bit)
            else:
                assert got == (0, [], -1), (pname, bit)


@pytest.mark.parametrize("name", list(CASES))
def test_mask_0_generates_the_text_from_before_the_knob(env, name):
    """Mask 0 hands the generator the 19-entry list of before; a pass in which the requested parts find no work
    generates that same text and key under any mask, so it shares its code object with mask 0."""
    C = ext()
    p0, p7 = _program(name, 0), _program(name, 7)
    for (pname, adjoint, j, ops, fidx), (_, _, _, ops7, fidx7) in zip(_passes(p0), _passes(p7)):
        c0, c7 = p0.spec_cfg(j, adjoint), p7.spec_cfg(j, adjoint)
        assert len(c0) == 19 and c7 == c0 + [7]
        s0, s7 = C.hea_spec_source(adjoint, ops, fidx, c0), C.hea_spec_source(adjoint, ops7, fidx7, c7)
        k0, k7 = (C.hea_spec_key(adjoint, ops, fidx, c, CSRC, ARCH) for c in (c0, c7))
        assert _marks(s0) == (0, [], -1)
        assert s0 == C.hea_spec_source(adjoint, ops, fidx, c0 + [0])
        assert k0 == C.hea_spec_key(adjoint, ops, fidx, c0 + [0], CSRC, ARCH)
        if CASES[name][1][pname][1][0]:
            assert s0 != s7 and k0 != k7
            # the knob adds its lines and changes nothing else
            kept = [ln for ln in s7.splitlines() if not re.match(r"#define QFX_HEA_SPEC_LEAN |constexpr int (NOBAR|EARLY_STORE)\b", ln)]
            assert kept == s0.splitlines()
        else:
            assert s0 == s7 and k0 == k7
