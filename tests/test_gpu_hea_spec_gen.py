"""The generating forward pass (pass 0 of an angle program: the layer-1 product state) compiled per plan
(``HeaMfmaProgram(spec_gen=True)`` / ``QFEDX_HEA_SPEC_GEN=1``) against the interpreter, BITWISE, and both against
digests recorded on the GPU at the commit before the generation's fp32 products were pinned in the source
(tests/golden/hea_gen_parent_digests.json, written by tools/hea_gen_digests.py, whose cases and step these tests import):
pinning must not move a bit of the interpreter, and the per-plan kernel must compute what the interpreter computes.

Compared: the stored pass-0 state, <Z>, the loss and the whole gradient.  Shapes (tools/hea_gen_digests.py CASES), the
smallest that reach each branch of the block: 8q x 1L (one tile of 2^8 amplitudes under 512 threads: wrapped table
reads, predicated stores), 10q x 2L on 2^8 tiles (qubits outside the tile: wave product, outer_s; four tiles), the
headline 16q x 3L plan and its 2^13 retiling; feature maps ry / rx / rz, fp16 and bf16, random angles, all-zero features
and parameters, x = pi.  Then one prefix-reuse parameter-shift call at 10q (shifted rows regenerate layer 1 in pass 0,
in_rep > 1), one evaluation (8q: generation and READOUT share a pass that stores no state) and one captured step
against the eager interpreter.  Every per-plan case asserts from ``spec_passes`` and the launch counters that pass 0
ran its per-plan kernel."""
import importlib.util
import json
import os

import pytest
import torch

from qfedx_amd.ops.hea_mfma import HeaMfmaProgram

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_sp = importlib.util.spec_from_file_location("hea_gen_digests", os.path.join(_ROOT, "tools", "hea_gen_digests.py"))
dg = importlib.util.module_from_spec(_sp)
_sp.loader.exec_module(dg)

with open(dg.GOLDEN) as _f:
    PARENT = json.load(_f)

MODES = {"interp": dict(use_spec=False), "perplan": dict(use_spec=True, spec_gen=True)}


@pytest.fixture(scope="module", autouse=True)
def _env(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("QFEDX_JIT_CACHE", str(tmp_path_factory.mktemp("hea_spec_gen_cache")))
    for name in ("QFEDX_HEA_SPLIT_RO", "QFEDX_HEA_SPEC", "QFEDX_HEA_SPEC_GEN", "QFEDX_DEBUG", "QFEDX_HEA_OBS_LOAD",
                 "QFEDX_HEA_ADJ_TILE", "QFEDX_HEA_TILE"):
        mp.delenv(name, raising=False)
    yield
    mp.undo()


_interp = {}


def _reference(name, dev):
    """The interpreter's step of a case, computed once and shared."""
    if name not in _interp:
        res, prog = dg.run_case(name, dev, **MODES["interp"])
        assert prog.spec_launches == 0 and prog.interp_launches > 0 and not any(prog.spec_passes()["fwd"])
        _interp[name] = res
    return _interp[name]


def _ran_per_plan(prog, steps=1):
    sp = prog.spec_passes()
    assert prog.spec_gen and sp["fwd"][0] is True and all(sp["fwd"]) and prog.spec_fwd[0] >= 0
    n_spec = sum(sp["fwd"]) + sum(sp["adj"])
    assert prog.spec_launches == steps * n_spec
    assert prog.interp_launches == steps * (len(sp["fwd"]) + len(sp["adj"]) - n_spec)


def test_cases_reach_the_branches():
    assert set(PARENT) == set(dg.CASES)
    shapes = {(n, L, t) for n, L, t, _, _, _ in dg.CASES.values()}
    assert shapes == {(8, 1, None), (10, 2, 8), (16, 3, None), (16, 3, 13)}
    assert {c[4] for c in dg.CASES.values()} == {"ry", "rx", "rz"} and {c[3] for c in dg.CASES.values()} == {"fp16", "bf16"}
    assert {c[5] for c in dg.CASES.values()} == {"random", "zero", "pi"}
    for name, (tiles, t, outside) in {"8q1L_ry": (1, 8, 0), "10q2L_t8_ry": (4, 8, 2), "16q3L_ry": (4, 14, 2),
                                      "16q3L_t13_ry": (8, 13, 3)}.items():
        prog = HeaMfmaProgram(dg.case_spec(name), "cpu", tile_bits=dg.CASES[name][2], use_spec=False)
        p = prog.passes[0][0]
        assert (1 << (prog.n - p.t), p.t, prog.n - p.t) == (tiles, t, outside) and prog._gen(0)


@pytest.mark.parametrize("name", list(dg.CASES))
def test_interpreter_keeps_the_parents_bits(cuda, name):
    got = dg.digests(_reference(name, cuda))
    print(name, got, "parent", PARENT[name])
    assert got == PARENT[name]


@pytest.mark.parametrize("name", list(dg.CASES))
def test_per_plan_pass0_is_bitwise_the_interpreter(cuda, name):
    ref = _reference(name, cuda)
    got, prog = dg.run_case(name, cuda, **MODES["perplan"])
    _ran_per_plan(prog)
    bad = {k: int((got[k] != ref[k]).sum()) for k in ref if not torch.equal(got[k], ref[k])}
    print(name, "mismatching entries:", bad, dg.digests(got))
    assert not bad and set(got) == {"psi0", "expz", "loss", "grad"}
    assert dg.digests(got) == PARENT[name]
    if dg.CASES[name][5] != "zero":
        assert got["grad"].abs().max() > 0
    assert (got["psi0"] != 0).any()


def test_knob_0_keeps_pass0_on_the_interpreter(cuda, monkeypatch):
    name = "10q2L_t8_ry"
    monkeypatch.setenv("QFEDX_HEA_SPEC_GEN", "0")
    res, prog = dg.run_case(name, cuda, use_spec=True)
    assert not prog.spec_gen and prog.spec_passes()["fwd"] == [False, True] and prog.spec_fwd[0] == -1
    assert prog.spec_launches > 0 and prog.interp_launches > 0
    monkeypatch.setenv("QFEDX_HEA_SPEC_GEN", "1")
    res1, prog1 = dg.run_case(name, cuda, use_spec=True)
    _ran_per_plan(prog1)
    for k in res:
        assert torch.equal(res[k], res1[k]) and torch.equal(res[k], _reference(name, cuda)[k])


def test_shifted_rows_regenerate_layer1_per_plan(cuda):
    """Prefix-reuse parameter shift: the branches of layer-1 parameters start at pass 0 with in_rep > 1 parameter rows
    per input sample."""
    name = "10q2L_t8_ry"
    spec = dg.case_spec(name)
    xang, _, _, params = dg.case_inputs(name, cuda)
    outs = {}
    for mode, kw in MODES.items():
        prog = HeaMfmaProgram(spec, cuda, tile_bits=8, **kw)
        l1 = {prog.plan.theta_slot(1, q) + d for q in range(spec.n_qubits) for d in (0, 1)}
        assert l1 <= set(prog.shift_owners()[0])                         # layer-1 rows start at the generating pass
        outs[mode] = prog.shifted_expz(xang[:1], params[:1], with_mean=True).clone()
        torch.cuda.synchronize()
        assert (prog.spec_launches > 0) == (mode == "perplan")
        if mode == "perplan":
            assert prog.spec_passes()["fwd"][0] is True
    assert torch.isfinite(outs["interp"]).all() and outs["interp"].abs().max() > 0
    assert torch.equal(outs["interp"], outs["perplan"])


def test_evaluation_generates_and_reads_out_in_one_pass(cuda):
    name = "8q1L_rz_pi"
    spec = dg.case_spec(name)
    xang, _, _, params = dg.case_inputs(name, cuda)
    outs = {}
    for mode, kw in MODES.items():
        prog = HeaMfmaProgram(spec, cuda, **kw)
        assert prog.n_passes == 1 and prog.fwd_last == 0
        outs[mode] = prog.expz(xang, params[:, : spec.n_theta].contiguous()).clone()
        torch.cuda.synchronize()
        assert (prog.spec_launches, prog.interp_launches) == ((1, 0) if mode == "perplan" else (0, 1))
    assert torch.isfinite(outs["interp"]).all() and torch.equal(outs["interp"], outs["perplan"])


def test_captured_step_equals_the_eager_interpreter(cuda):
    """One step with pass 0 per plan, recorded into a graph and replayed twice."""
    name = "16q3L_ry"
    spec = dg.case_spec(name)
    xang, y, w, params = dg.case_inputs(name, cuda)
    ref = _reference(name, cuda)
    prog = HeaMfmaProgram(spec, cuda, **MODES["perplan"])
    ws = {}
    with prog.private_workspace(ws):
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            prog.loss_and_grads(xang, y, w, params, spec)
        torch.cuda.current_stream(cuda).wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out = prog.loss_and_grads(xang, y, w, params, spec)
    for _ in range(2):
        gr.replay()
    torch.cuda.synchronize()
    assert prog.spec_passes() == {"fwd": [True, True], "adj": [True, False]} and prog.spec_launches > 0
    for k in ("expz", "loss", "grad"):
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(ws["psi0"][: (dg.K * dg.B) << spec.n_qubits], ref["psi0"])
