"""The lean per-plan kernels (``HeaMfmaProgram.spec_lean`` = 7: held im-row fragments in the adjoint pair ops, no op
barrier between cross-only gradient ops, tile stores issued ahead of a read-only tail) against the same kernels without
the knob (``spec_lean`` = 0) and against the interpreter (``use_spec=False``), BITWISE: <Z>, loss, hits and the whole
gradient of a training step, the state the last forward pass stores, every stored lambda, and the <Z> of an evaluation
(whose last forward pass stores nothing).

Shapes, the smallest that reach each path (op lists: tests/test_hea_spec_lean.py):
  8q x 2L    tile 2^8: one partial block per wave; two adjacent GRAD_L1 (a dropped barrier)
  11q x 2L   tile 2^11: the smallest pair tile; BACK2, then GRAD2 and GRAD_L1 adjacent
  13q x 2L   tile 2^13: the full adjoint tile; GRAD2, GRAD2
  14q x 2L   tiles 2^13 / 2^13: two passes, two tiles per sample; the lambda-storing pass ends BACK, GRAD_L1
  16q x 3L   tiles 2^14 / 2^13: the headline plan, 6 samples
fp16 and bf16 storage.  The split readout is forced on, so the last adjoint pass runs per plan too; every case asserts
from the launch counters that every pass ran its per-plan kernel.  Every step runs twice (equal results), and one
captured step is replayed twice."""
import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram

pytestmark = pytest.mark.gpu

MODES = {"interp": None, "lean0": 0, "lean7": 7}
# name: (qubits, layers, forward tile bits, clients, batch)
SHAPES = {"8q2L": (8, 2, None, 2, 3), "11q2L": (11, 2, None, 2, 3), "13q2L": (13, 2, None, 2, 2),
          "14q2L_t13": (14, 2, 13, 2, 2), "16q3L": (16, 3, None, 2, 3)}


@pytest.fixture(scope="module", autouse=True)
def _tmp_cache(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("QFEDX_JIT_CACHE", str(tmp_path_factory.mktemp("hea_spec_lean_cache")))
    for name in ("QFEDX_HEA_SPLIT_RO", "QFEDX_HEA_SPEC", "QFEDX_HEA_SPEC_GEN", "QFEDX_HEA_SPEC_LEAN", "QFEDX_DEBUG",
                 "QFEDX_HEA_OBS_LOAD", "QFEDX_HEA_ADJ_TILE", "QFEDX_HEA_TILE", "QFEDX_HEA_NT"):
        mp.delenv(name, raising=False)
    yield
    mp.undo()


def _program(name, dev, mode, storage):
    n, L, tile, _, _ = SHAPES[name]
    lean = MODES[mode]
    prog = HeaMfmaProgram(VQCSpec(n, L, 3), dev, tile_bits=tile, storage=storage, use_spec=lean is not None,
                          spec_gen=True, spec_lean=lean or 0)
    prog.split_readout = True
    if lean is None:
        assert not prog.spec_active
    else:
        assert prog.spec_lean == lean and all(h >= 0 for h in prog.spec_fwd[: prog.fwd_last + 1] + prog.spec_adj)
    return prog


def _inputs(name, dev):
    n, L, _, K, B = SHAPES[name]
    spec = VQCSpec(n, L, 3)
    g = torch.Generator().manual_seed(29)
    xang = spec.encode_features(torch.rand(K, B, n, generator=g)).to(dev)
    y = torch.randint(0, 3, (K, B), generator=g).to(dev)
    w = torch.rand(K, B, generator=g) / B
    params = torch.stack([spec.init_params(k) for k in range(K)])
    params = (params + 0.3 * torch.randn(params.shape, generator=g)).to(dev)
    return spec, xang, y, w.to(dev), params


def _step(prog, spec, xang, y, w, params):
    """One training step -> its outputs and the states it leaves in the workspaces."""
    K, B = w.shape
    S, n = K * B, prog.n
    out = prog.loss_and_grads(xang, y, w, params, spec)
    res = {k: out[k].clone() for k in ("loss", "correct", "grad", "expz")}
    res["psi_last"] = prog._ws[f"psi{prog.fwd_last}"][: S << n].clone()
    for nm, t in prog._ws.items():
        if nm.startswith("lam"):
            res["state_" + nm] = t[: S << n].clone()
    return res


def _run(name, dev, mode, storage):
    spec, xang, y, w, params = _inputs(name, dev)
    prog = _program(name, dev, mode, storage)
    first = _step(prog, spec, xang, y, w, params)
    again = _step(prog, spec, xang, y, w, params)
    ev = prog.expz(xang, params[:, : spec.n_theta].contiguous())
    torch.cuda.synchronize()
    J, R = prog.n_passes, prog.fwd_last
    if mode == "interp":
        assert prog.spec_launches == 0
    else:
        assert prog.readout_mode(w.numel()) == "split"
        assert (prog.spec_launches, prog.interp_launches) == (2 * (R + 1 + J) + R + 1, 0)
    assert not _mismatches(again, first)                    # two runs of the same step
    first["eval_expz"] = ev.clone()
    return first, prog


def _mismatches(got, ref):
    assert set(got) == set(ref)
    return {k: int((got[k] != ref[k]).sum()) for k in ref if not torch.equal(got[k], ref[k])}


@pytest.fixture(scope="module")
def results(cuda):
    """(shape, storage) -> mode -> (results, program), each computed once."""
    memo = {}

    def get(name, storage):
        if (name, storage) not in memo:
            memo[name, storage] = {m: _run(name, cuda, m, storage) for m in MODES}
        return memo[name, storage]
    return get


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_lean_kernels_are_bitwise(results, name, storage):
    out = results(name, storage)
    res, prog = out["lean7"]
    n, L, tile, K, B = SHAPES[name]
    tiles = [(e.fwd_pass.t, e.adj_pass.t) for e in prog.passes]
    assert tiles == {"8q2L": [(8, 8)], "11q2L": [(11, 11)], "13q2L": [(13, 13)], "14q2L_t13": [(13, 13)] * 2,
                     "16q3L": [(14, 13)] * 2}[name]
    assert ("state_lam1" in res) == (prog.n_passes == 2)    # the pass that stores lambda ahead of its last op
    assert torch.isfinite(res["grad"]).all() and res["grad"].abs().max() > 0 and res["psi_last"].ne(0).any()
    for ref in ("lean0", "interp"):
        bad = _mismatches(res, out[ref][0])
        print(name, storage, "lean7 vs", ref, "mismatching entries:", bad)
        assert not bad


@pytest.mark.parametrize("name", ["14q2L_t13", "16q3L"])
def test_a_captured_step_replays_bitwise(cuda, results, name):
    ref, _ = results(name, "fp16")["interp"]
    spec, xang, y, w, params = _inputs(name, cuda)
    prog = _program(name, cuda, "lean7", "fp16")            # (its kernels are compiled already: shared by key)
    ws = {}
    with prog.private_workspace(ws):
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            _step(prog, spec, xang, y, w, params)
        torch.cuda.current_stream(cuda).wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            got = _step(prog, spec, xang, y, w, params)
    for _ in range(2):
        for t in got.values():
            t.fill_(0)
        gr.replay()
        torch.cuda.synchronize()
        assert not _mismatches(got, {k: ref[k] for k in got})
