"""Seeding tile load of the per-plan last adjoint pass (``HeaMfmaProgram.obs_at_load``, csrc/hea_mfma.hip seed_tile_il),
the parts that need no GPU: with the flag on the generated text compiles for gfx950 within the resource bounds of
``test_hea_spec.py``, only the pass that starts with the observable op changes its text and cache key, and with the
flag off the generated text is what it was before the flag existed (no trace of it)."""
import os
import re
import shutil
import subprocess

import pytest

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_plan as hp
from qfedx_amd.ops._ext import ext
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
from qfedx_amd.ops.statevec_hip import ARCH, CSRC

# name: (qubits, layers, classes, storage); 16q3L: two passes, the last adjoint pass on 2^13 tiles.  (Four classes,
# not the three of test_hea_spec.py's plans: compiled kernels are shared in-process by key, and that file looks for the
# code objects of its own plans in its own cache directories.)
CASES = {"8q2L": (8, 2, 4, "fp16"), "8q2L_bf16": (8, 2, 4, "bf16"), "16q3L": (16, 3, 4, "fp16"),
         "16q3L_bf16": (16, 3, 4, "bf16"), "10q3L_C8": (10, 3, 8, "fp16")}


def _program(name, flag):
    n, L, C, storage = CASES[name]
    spec = VQCSpec(n, L, C, readout_scale=2.0)
    prog = HeaMfmaProgram(spec, "cpu", storage=storage, use_spec=False)
    prog.obs_at_load = bool(flag)
    return prog


def _passes(prog):
    """(pass index, adjoint, ops, fidx) of every pass program that has a per-plan kernel."""
    for j, ((f, ff), (a, fa)) in enumerate(prog._host_progs):
        if 0 < j <= prog.fwd_last and len(f):
            yield j, False, f, ff
        if len(a):
            yield j, True, a, fa


def _readelf():
    cands = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"),
             shutil.which("llvm-readelf")]
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise RuntimeError("llvm-readelf of the ROCm toolchain not found")


def _metadata(path):
    out = subprocess.run([_readelf(), "--notes", path], capture_output=True, text=True, check=True).stdout
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, out).group(1))
            for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """Every case's kernels with the flag on, compiled once into a temporary cache: name -> (program, cache dir)."""
    out = {}
    mp = pytest.MonkeyPatch()
    try:
        for name in CASES:
            cache = str(tmp_path_factory.mktemp("obs_" + name))
            mp.setenv("QFEDX_JIT_CACHE", cache)
            prog = _program(name, 1)
            assert prog.prepare_spec(), name
            out[name] = (prog, cache)
    finally:
        mp.undo()
    return out


def test_the_knob_is_read_when_the_program_is_built(monkeypatch):
    for env, want in (("0", False), ("1", True)):
        monkeypatch.setenv("QFEDX_HEA_OBS_LOAD", env)
        prog = HeaMfmaProgram(VQCSpec(8, 2, 3), "cpu", use_spec=False)
        assert prog.obs_at_load is want
        assert prog.spec_cfg(0, True)[18] == int(want) and len(prog.spec_cfg(0, True)) == 19


@pytest.mark.parametrize("name", list(CASES))
def test_seeding_kernels_compile_within_the_resource_bounds(compiled, name):
    """One kernel per pass as before; no scratch, <= 128 VGPRs, LDS <= 81,920 B on tiles up to 2^13; and the last
    adjoint pass's text carries the seeding load."""
    prog, cache = compiled[name]
    C = ext()
    J = prog.n_passes
    assert prog.spec_adj[J - 1] >= 0
    assert sum(h >= 0 for h in prog.spec_fwd + prog.spec_adj) == prog.fwd_last + J == len(prog.spec_keys)
    a, fa = prog._host_progs[J - 1][1]
    assert int(a[0, hp.W_CODE]) == hp.OP_OBS
    assert "#define QFX_HEA_OBS_LOAD 1" in C.hea_spec_source(True, a, fa, prog.spec_cfg(J - 1, True))
    if name.startswith("16q3L"):
        assert (J, prog.passes[J - 1][3].t) == (2, 13)
    for j, h in enumerate(prog.spec_adj):
        path = os.path.join(cache, "probe.co")
        with open(path, "wb") as f:
            f.write(C.hea_spec_code(h))
        md = _metadata(path)
        print(name, "adj", j, md)
        assert md["private_segment_fixed_size"] == 0
        assert md["vgpr_count"] <= 128
        if prog.passes[j][3].t <= 13:
            assert md["group_segment_fixed_size"] <= 81920


@pytest.mark.parametrize("name", list(CASES))
def test_only_the_pass_that_starts_with_obs_changes(name):
    """Flag 1 against flag 0: another text and key for the last adjoint pass; the same text and key for every pass
    that does not start with the observable op (so those still share their cache entries, as
    test_hea_spec.test_cache_key_follows_the_plan asserts for the two 16-qubit tilings)."""
    C = ext()
    p0, p1 = _program(name, 0), _program(name, 1)
    J = p0.n_passes
    seen_other = 0
    for (j, adjoint, ops, fidx), (_, _, ops1, fidx1) in zip(_passes(p0), _passes(p1)):
        c0, c1 = p0.spec_cfg(j, adjoint), p1.spec_cfg(j, adjoint)
        assert c0[:18] == c1[:18] and (c0[18], c1[18]) == (0, 1)
        s0, s1 = C.hea_spec_source(adjoint, ops, fidx, c0), C.hea_spec_source(adjoint, ops1, fidx1, c1)
        k0, k1 = (C.hea_spec_key(adjoint, ops, fidx, c, CSRC, ARCH) for c in (c0, c1))
        starts_obs = int(ops[0, hp.W_CODE]) == hp.OP_OBS
        assert starts_obs == (adjoint and j == J - 1)
        if starts_obs:
            assert s0 != s1 and k0 != k1
            assert s1.replace("#define QFX_HEA_OBS_LOAD 1\n", "") == s0
        else:
            assert s0 == s1 and k0 == k1
            seen_other += 1
    assert seen_other or J == 1


@pytest.mark.parametrize("name", list(CASES))
def test_flag_off_generates_the_text_from_before_the_flag(name):
    """The configuration list grew by one entry, so the key inputs of flag 0 are shown unchanged through the text: the
    18-entry list of before and the 19-entry list with the flag off give the same generated text and the same key, and
    that text does not mention the flag (hea_mfma.hip then defines it 0: the tile load and the op loop of before)."""
    C = ext()
    prog = _program(name, 0)
    for j, adjoint, ops, fidx in _passes(prog):
        cfg = prog.spec_cfg(j, adjoint)
        assert len(cfg) == 19 and cfg[18] == 0
        src = C.hea_spec_source(adjoint, ops, fidx, cfg)
        assert src == C.hea_spec_source(adjoint, ops, fidx, cfg[:18])
        assert "OBS_LOAD" not in src
        assert C.hea_spec_key(adjoint, ops, fidx, cfg, CSRC, ARCH) == C.hea_spec_key(adjoint, ops, fidx, cfg[:18], CSRC, ARCH)
