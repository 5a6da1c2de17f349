"""Per-plan MFMA pass kernels (csrc/hea_spec.cpp), the parts that need no GPU: the XOR bases the generated prelude
carries rebuild every address table of the planner, the generated text compiles with hiprtc for gfx950, the cache key
follows the plan, and every compiled kernel keeps the resource bounds that let two workgroups share a CU."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_plan as hp
from qfedx_amd.ops._ext import ext
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
from qfedx_amd.ops.statevec_hip import ARCH, CSRC

# (qubits, layers, forward tile bits)
PLANS = [(8, 2, 14), (10, 2, 14), (11, 3, 14), (12, 3, 14), (16, 3, 14), (16, 3, 13), (18, 2, 14), (20, 2, 14),
         (24, 3, 14)]


@functools.lru_cache(maxsize=None)
def _program(n, L, tile=14, storage="fp16"):
    return HeaMfmaProgram(VQCSpec(n_qubits=n, n_layers=L, n_classes=3), "cpu", tile_bits=tile, storage=storage,
                          use_spec=False)


def _basis_table(basis, nb):
    out = np.zeros(1 << nb, dtype=np.int64)
    for i in range(1 << nb):
        for j in range(nb):
            if (i >> j) & 1:
                out[i] ^= basis[j]
    return out


@pytest.mark.parametrize("n,L,tile", PLANS)
def test_address_tables_are_their_xor_bases(n, L, tile):
    """tab[i] = XOR_j bit_j(i) tab[1 << j] for the OFF / OFF2 / BL / BH table of every group-op record, and the bases
    in the generated prelude are exactly tab[1 << j]."""
    prog = _program(n, L, tile)
    C = ext()
    checked = 0
    for j, ((f, ff), (a, fa)) in enumerate(prog._host_progs):
        for adjoint, ops, fidx in ((False, f, ff), (True, a, fa)):
            if not len(ops):
                continue
            src = C.hea_spec_source(adjoint, ops, fidx, prog.spec_cfg(j, adjoint))
            emitted = {}
            for name, nb in (("OFFB", 4), ("OFF2B", 4), ("BLB", 5), ("BHB", 5)):
                m = re.search(r"constexpr unsigned %s\[NOPS\]\[%d\] = \{(.*)\};" % (name, nb), src)
                vals = [int(v) for v in re.findall(r"(\d+)u", m.group(1))]
                emitted[name] = np.array(vals, dtype=np.int64).reshape(len(ops), nb)
            for o, w in enumerate(ops.numpy().astype(np.int64)):
                code = int(w[hp.W_CODE])
                if code in (hp.OP_OBS, hp.OP_READOUT):
                    continue
                tabs = [("OFFB", hp.W_OFF, 4), ("BLB", hp.W_BL, 5), ("BHB", hp.W_BH, 5)]
                if code in (hp.OP_APPLY2, hp.OP_BACK2, hp.OP_GRAD2):
                    tabs.append(("OFF2B", hp.W_OFF2, 4))
                for name, word, nb in tabs:
                    tab = w[word:word + (1 << nb)]
                    basis = [int(tab[1 << b]) for b in range(nb)]
                    assert tab[0] == 0
                    assert np.array_equal(_basis_table(basis, nb), tab), (j, adjoint, o, name)
                    assert list(emitted[name][o]) == basis
                    checked += 1
    assert checked > 0


# ---------------------------------------------------------------------------------------------- compiled kernels
CASES = {"8q2L": (8, 2, 14, "fp16"), "11q3L": (11, 3, 14, "fp16"), "16q3L": (16, 3, 14, "fp16"),
         "16q3L_bf16": (16, 3, 14, "bf16"), "16q3L_t13": (16, 3, 13, "fp16")}


def _readelf():
    cands = [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"),
             shutil.which("llvm-readelf")]
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise RuntimeError("llvm-readelf of the ROCm toolchain not found")


def _metadata(path):
    out = subprocess.run([_readelf(), "--notes", path], capture_output=True, text=True, check=True).stdout

    def field(name):
        return int(re.search(r"\.%s:\s+(\d+)" % name, out).group(1))
    return {k: field(k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """Every case's forward and adjoint kernels, compiled once into a temporary cache: name -> (program, cache dir)."""
    out = {}
    saved = os.environ.get("QFEDX_JIT_CACHE")
    try:
        for name, (n, L, tile, storage) in CASES.items():
            cache = str(tmp_path_factory.mktemp("spec_" + name))
            os.environ["QFEDX_JIT_CACHE"] = cache
            prog = _program(n, L, tile, storage)
            assert prog.prepare_spec(), name
            out[name] = (prog, cache)
    finally:
        if saved is None:
            os.environ.pop("QFEDX_JIT_CACHE", None)
        else:
            os.environ["QFEDX_JIT_CACHE"] = saved
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_generated_text_compiles_for_gfx950(compiled, name):
    prog, cache = compiled[name]
    assert prog.spec_active
    n_kernels = sum(h >= 0 for h in prog.spec_fwd + prog.spec_adj)
    # (forward pass 0, the layer-1 generation, stays on the interpreter)
    assert prog.spec_fwd[0] == -1
    assert n_kernels == prog.fwd_last + prog.n_passes and n_kernels == len(prog.spec_keys)
    # (a kernel an earlier case already compiled - the 2^13 adjoint passes of both 16-qubit tilings are one plan -
    # is reused in-process and sits in that case's cache directory)
    dirs = [c for _, c in compiled.values()]
    for key in prog.spec_keys:
        found = [d for d in dirs if os.path.exists(os.path.join(d, key + ".co"))]
        assert found, key
        assert os.path.getsize(os.path.join(found[0], key + ".co")) > 0
        with open(os.path.join(found[0], key + ".hip")) as f:
            assert "#define QFX_HEA_SPEC 1" in f.read()
    if name == "16q3L":
        assert (prog.passes[0][0].t, prog.adj_tile_bits) == (14, 13)
    if name == "16q3L_t13":
        assert prog.passes[0][0].t == 13


@pytest.mark.parametrize("name", list(CASES))
def test_compiled_kernels_keep_the_resource_bounds(compiled, name):
    """No scratch, <= 128 VGPRs, and LDS that leaves room for two workgroups per CU (160 KB): <= 81,920 B for the
    adjoint on tiles up to 2^13, <= 78,336 B for the forward."""
    prog, cache = compiled[name]
    C = ext()
    for handles, adjoint in ((prog.spec_fwd, False), (prog.spec_adj, True)):
        for j, h in enumerate(handles):
            if h < 0:
                continue
            path = os.path.join(cache, "probe.co")
            with open(path, "wb") as f:
                f.write(C.hea_spec_code(h))
            md = _metadata(path)
            print(name, "adj" if adjoint else "fwd", j, md)
            assert md["private_segment_fixed_size"] == 0
            assert md["vgpr_count"] <= 128
            t = prog.passes[j][3].t if adjoint else prog.passes[j][0].t
            if adjoint and t <= 13:
                assert md["group_segment_fixed_size"] <= 81920
            if not adjoint:
                assert md["group_segment_fixed_size"] <= 78336


def _keys(n, L, tile=14, storage="fp16", stamps=0):
    """(forward keys, adjoint keys) of a plan's pass kernels."""
    prog = _program(n, L, tile, storage)
    C = ext()
    keys = ([], [])
    for j, ((f, ff), (a, fa)) in enumerate(prog._host_progs):
        for adjoint, ops, fidx in ((False, f, ff), (True, a, fa)):
            if len(ops) and (adjoint or j <= prog.fwd_last):
                cfg = prog.spec_cfg(j, adjoint)
                cfg[16] = stamps
                keys[adjoint].append(C.hea_spec_key(adjoint, ops, fidx, cfg, CSRC, ARCH))
    return keys


def test_cache_key_follows_the_plan():
    bf, ba = _keys(16, 3)
    assert (bf, ba) == _keys(16, 3)
    assert len(set(bf + ba)) == len(bf + ba)               # every pass kernel its own entry
    for of, oa in (_keys(12, 3), _keys(16, 2), _keys(16, 3, storage="bf16"), _keys(16, 3, stamps=1)):
        assert not set(bf + ba) & set(of + oa)
    # forward tile bits 13 instead of 14: other forward kernels; the adjoint runs on 2^13 tiles under both, the same
    # compiled text, so it shares the entries
    of, oa = _keys(16, 3, tile=13)
    assert not set(bf) & set(of) and oa == ba


def test_nonlinear_table_is_refused():
    """A record whose table is not XOR-linear cannot be specialised: the generator raises (the program then stays on
    the interpreter) instead of emitting wrong addresses."""
    prog = _program(8, 2)
    f, ff = prog._host_progs[0][0]
    bad = f.clone()
    bad[0, hp.W_OFF + 3] ^= 1
    with pytest.raises(RuntimeError, match="XOR-linear"):
        ext().hea_spec_source(False, bad, ff, prog.spec_cfg(0, False))
