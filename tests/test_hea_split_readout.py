"""Which readout route a training step of the MFMA engine takes (``HeaMfmaProgram.readout_mode``; no GPU needed): the
split route only for noiseless steps that would otherwise fuse, whose last adjoint pass has a per-plan kernel, from
``SPLIT_READOUT_MIN_SAMPLES`` samples on; ``split_readout`` / ``QFEDX_HEA_SPLIT_RO`` replace the sample-count rule only;
``spec_passes()`` without a sample count keeps its meaning."""
import pytest

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_mfma
from qfedx_amd.ops.hea_mfma import SPLIT_READOUT_MIN_SAMPLES as S_MIN
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram


@pytest.fixture()
def env(monkeypatch):
    for name in ("QFEDX_HEA_SPLIT_RO", "QFEDX_HEA_SPEC", "QFEDX_DEBUG"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _prog(n=8, L=2, C=3, use_spec=False):
    """A program on the CPU.  ``use_spec=False`` compiles nothing; ``_with_kernels`` then stands in for prepared
    per-plan kernels (the rule only asks whether the last adjoint pass has a handle), so this file never puts a plan
    of another test file into the process-wide kernel table."""
    return HeaMfmaProgram(VQCSpec(n_qubits=n, n_layers=L, n_classes=C), "cpu", use_spec=use_spec)


def _with_kernels(prog):
    prog.spec_adj = [0] * prog.n_passes
    return prog


def test_selection_rule(env):
    assert S_MIN >= 64                                   # (steps of a few samples stay fused whatever was measured)
    prog = _with_kernels(_prog())
    assert prog.split_readout is None and prog.spec_active and prog.spec_adj[-1] >= 0
    assert prog.readout_mode(S_MIN) == "split" and prog.readout_mode(100 * S_MIN) == "split"
    assert prog.readout_mode(S_MIN - 1) == "fused" and prog.readout_mode(6) == "fused"
    assert prog.readout_mode() == "fused"
    # readout noise, or the fused readout switched off: the readout kernel, at any sample count
    assert prog.readout_mode(S_MIN, noise=object()) == "kernel"
    prog.fused_readout = False
    assert prog.readout_mode(S_MIN) == "kernel"
    prog.fused_readout = True
    # the knob replaces the sample-count rule, and nothing else
    prog.split_readout = True
    assert prog.readout_mode(1) == "split" and prog.readout_mode() == "fused"
    assert prog.readout_mode(1, noise=object()) == "kernel"
    prog.split_readout = False
    assert prog.readout_mode(100 * S_MIN) == "fused"
    # without a per-plan kernel for the last adjoint pass there is nothing to gain: fused
    prog.split_readout = True
    prog.spec_adj = [-1] * prog.n_passes
    assert prog.readout_mode(S_MIN) == "fused"


def test_spec_passes_keeps_its_meaning(env):
    prog = _with_kernels(_prog())                        # one pass: first and last
    assert prog.spec_passes() == {"fwd": [False], "adj": [False]}
    assert prog.spec_passes(True) == {"fwd": [False], "adj": [False]}
    assert prog.spec_passes(False) == {"fwd": [False], "adj": [True]}
    assert prog.spec_passes(samples=S_MIN - 1) == prog.spec_passes()
    assert prog.spec_passes(samples=S_MIN) == {"fwd": [False], "adj": [True]}
    assert prog.spec_passes(True, samples=S_MIN) == {"fwd": [False], "adj": [True]}
    assert prog.spec_passes(False, samples=6) == {"fwd": [False], "adj": [True]}


def test_env_knobs(env):
    env.setenv("QFEDX_HEA_SPEC", "0")                    # the interpreter everywhere: every step fuses
    off = _prog(use_spec=None)
    assert not off.spec_requested and not off.spec_active and off.readout_mode(100 * S_MIN) == "fused"
    off.split_readout = True
    assert off.readout_mode(100 * S_MIN) == "fused"
    env.setenv("QFEDX_HEA_SPEC", "1")
    env.setenv("QFEDX_HEA_SPLIT_RO", "0")
    assert hea_mfma.split_readout_default() is False
    assert hea_mfma.spec_default()
    p0 = _with_kernels(_prog())
    assert p0.split_readout is False and p0.readout_mode(100 * S_MIN) == "fused"
    env.setenv("QFEDX_HEA_SPLIT_RO", "1")
    p1 = _with_kernels(_prog())
    assert p1.split_readout is True and p1.readout_mode(1) == "split"
    env.delenv("QFEDX_HEA_SPLIT_RO")
    assert hea_mfma.split_readout_default() is None


def test_more_than_64_partials_per_sample_is_not_split(env):
    """20 qubits x 8 classes: 64 readout tiles x 8 = 512 partials per sample - the readout kernel, as before."""
    prog = _with_kernels(_prog(20, 2, 8))                # (even with per-plan kernels)
    assert prog.tiles_last * prog.C > 64
    prog.split_readout = True
    assert prog.readout_mode(S_MIN) == "kernel"
