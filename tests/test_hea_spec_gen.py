"""Which kernel the generating forward pass (pass 0 of an angle program) gets: ``HeaMfmaProgram.spec_gen`` /
``QFEDX_HEA_SPEC_GEN`` and what ``spec_passes()`` reports for it (no GPU needed: hiprtc compiles for gfx950 here).
A program built directly keeps pass 0 on the interpreter unless asked; the engine asks (``SPEC_GEN_ENGINE``); the
environment variable overrides both; amplitude programs have no generating pass and do not change."""
import pytest

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_mfma
from qfedx_amd.ops._ext import ext
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram, spec_gen_default


@pytest.fixture()
def env(monkeypatch, tmp_path):
    for name in ("QFEDX_HEA_SPLIT_RO", "QFEDX_HEA_SPEC", "QFEDX_HEA_SPEC_GEN", "QFEDX_DEBUG", "QFEDX_STAMPS",
                 "QFEDX_EXTRA_HIPFLAGS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("QFEDX_JIT_CACHE", str(tmp_path))
    return monkeypatch


def _prog(env=None, **kw):
    return HeaMfmaProgram(VQCSpec(n_qubits=10, n_layers=2, n_classes=3), "cpu", tile_bits=8, **kw)


def test_knob(env):
    assert hea_mfma.SPEC_GEN_ENGINE is True
    assert spec_gen_default() is False and spec_gen_default(True) is True      # unset: the caller decides
    env.setenv("QFEDX_HEA_SPEC_GEN", "0")
    assert spec_gen_default() is False and spec_gen_default(True) is False
    env.setenv("QFEDX_HEA_SPEC_GEN", "1")
    assert spec_gen_default() is True and spec_gen_default(True) is True
    assert _prog(use_spec=False).spec_gen is True                              # read when the program is built
    assert _prog(use_spec=False, spec_gen=False).spec_gen is False             # an explicit argument wins


def test_engine_asks_for_it(env):
    """The engine builds its MFMA program with the knob on; the environment variable still overrides."""
    from qfedx_amd.ops.engine import VQCEngine
    seen = []

    class Recorder:
        def __init__(self, *a, **kw):
            seen.append(kw)

    env.setattr(hea_mfma, "HeaMfmaProgram", Recorder)
    VQCEngine(VQCSpec(n_qubits=8, n_layers=1, n_classes=3), "cpu", "hip", "mfma")
    env.setenv("QFEDX_HEA_SPEC_GEN", "0")
    VQCEngine(VQCSpec(n_qubits=8, n_layers=1, n_classes=3), "cpu", "hip", "mfma_bf16")
    assert [kw["spec_gen"] for kw in seen] == [True, False] and seen[1]["storage"] == "bf16"


def test_spec_passes_reports_pass0(env):
    off = _prog(use_spec=True)
    assert off.n_passes == 2 and off._gen(0) and not off._gen(1)
    assert off.spec_gen is False and off.spec_fwd[0] == -1 and off.spec_fwd[1] >= 0
    assert off.spec_passes()["fwd"] == [False, True]
    on = _prog(use_spec=True, spec_gen=True)
    assert on.spec_gen is True and on.spec_fwd[0] >= 0 and on.spec_passes()["fwd"] == [True, True]
    assert on.spec_passes()["adj"] == off.spec_passes()["adj"]
    assert on.spec_fwd[1] == off.spec_fwd[1] and on.spec_adj == off.spec_adj      # every other pass: the same kernels
    interp = _prog(use_spec=False, spec_gen=True)                                   # nothing compiled: nothing per plan
    assert interp.spec_passes()["fwd"] == [False, False] and not interp.spec_active


def test_pass0_text_has_the_generation_constants(env):
    prog = _prog(use_spec=False)
    (f, ff), _ = prog._host_progs[0]
    cfg = prog.spec_cfg(0, False)
    assert cfg[6] == 1 and prog.spec_cfg(1, False)[6] == 0
    text = ext().hea_spec_source(False, f, ff, cfg)
    p = prog.passes[0][0]
    assert "GEN = 1" in text and f"N = 10, T = {p.t}, CB = {p.c}, LO = {p.lo}, HI = {p.hi}" in text


def test_amplitude_programs_do_not_change(env):
    spec = VQCSpec(n_qubits=8, n_layers=1, n_classes=3, feature_map="amplitude")
    a = HeaMfmaProgram(spec, "cpu", use_spec=True, spec_gen=False)
    b = HeaMfmaProgram(spec, "cpu", use_spec=True, spec_gen=True)
    assert not a._gen(0) and a.spec_fwd == b.spec_fwd and a.spec_adj == b.spec_adj and a.spec_fwd[0] >= 0
