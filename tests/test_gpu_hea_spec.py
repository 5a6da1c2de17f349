"""Per-plan MFMA pass kernels (csrc/hea_spec.cpp) against the interpreter (csrc/hea_mfma.hip), BITWISE: the two builds
compile the same pass bodies, so <Z>, loss, hits, parameter gradients and every stored pass state must be identical.
Shapes: the smallest that reach each code path (one partial-tile pass; the smallest pair-op plan; the headline two-pass
plan in fp16 and bf16; its 2^13 forward tiling; four passes with middle passes that load and store both states;
shifted parameter rows sharing an input sample; launches recorded into a graph).

Two passes run on the interpreter under both settings: the layer-1 generation pass (forward pass 0) and the last adjoint
pass while it computes the fused readout (ops/hea_mfma.py).  A single-pass plan therefore launches a per-plan kernel only
in a step WITHOUT the fused readout, so every shape runs with ``fused_readout = False`` on both sides (the last adjoint
pass, with its OBS op, then runs per plan), the multi-pass shapes also with it, and every case asserts that per-plan
kernels were actually launched (``spec_launches``)."""
import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram, spec_default

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _tmp_cache(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("QFEDX_JIT_CACHE", str(tmp_path_factory.mktemp("hea_spec_cache")))
    yield
    mp.undo()


def _inputs(spec, K, B, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    n = spec.n_qubits
    xang = spec.encode_features(torch.rand(K, B, n, generator=g)).to(dev)
    y = torch.randint(0, spec.n_classes, (K, B), generator=g).to(dev)
    w = torch.full((K, B), 1.0 / B, device=dev)
    params = torch.stack([spec.init_params(k) for k in range(K)])
    params = (params + 0.3 * torch.randn(params.shape, generator=g)).to(dev)
    return xang, y, w, params


def _step(spec, dev, K, B, use_spec, tile=None, storage="fp16", fused=True):
    """One training step -> its outputs and every stored pass state (psi of each forward pass, lambda of each adjoint
    pass: the int32 workspaces)."""
    xang, y, w, params = _inputs(spec, K, B, dev)
    prog = HeaMfmaProgram(spec, dev, tile_bits=tile, storage=storage, use_spec=use_spec)
    assert prog.spec_active == use_spec
    prog.fused_readout = fused
    out = prog.loss_and_grads(xang, y, w, params, spec)
    torch.cuda.synchronize()
    # what ran: the passes spec_passes names, counted at the launches
    sp = prog.spec_passes(fused)
    n_spec = sum(sp["fwd"]) + sum(sp["adj"])
    assert prog.spec_launches == n_spec and prog.interp_launches == len(sp["fwd"]) + len(sp["adj"]) - n_spec
    assert (prog.spec_launches > 0) == use_spec
    res = {k: out[k].clone() for k in ("loss", "correct", "grad", "expz")}
    S = K * B
    for name, t in prog._ws.items():
        if name.startswith(("psi", "lam")):
            res["state_" + name] = t[: S << spec.n_qubits].clone()
    return res, prog


SHAPES = {
    "8q2L": (8, 2, 2, 3, None, "fp16"),         # one pass, partial tile, idle waves: OBS / BACK / GRAD_L1 per plan
    "11q3L": (11, 3, 2, 2, None, "fp16"),       # smallest plan with pair ops: OBS / BACK2 / GRAD2 per plan
    "16q3L": (16, 3, 2, 3, None, "fp16"),       # headline: two passes, 2^14 forward tiles, 2^13 adjoint tiles
    "16q3L_bf16": (16, 3, 2, 3, None, "bf16"),
    "16q3L_t13": (16, 3, 2, 3, 13, "fp16"),     # the small-batch forward tiling
    "18q4L": (18, 4, 1, 2, None, "fp16"),       # four passes: middle passes load and store both psi and lambda
}


@pytest.mark.parametrize("name,fused", [(nm, False) for nm in SHAPES] +
                         [(nm, True) for nm in ("16q3L", "16q3L_bf16", "16q3L_t13")])
def test_spec_step_is_bitwise_the_interpreter(cuda, name, fused):
    n, L, K, B, tile, storage = SHAPES[name]
    spec = VQCSpec(n, L, 3)
    ref, _ = _step(spec, cuda, K, B, False, tile, storage, fused)
    got, prog = _step(spec, cuda, K, B, True, tile, storage, fused)
    assert set(got) == set(ref) and any(k.startswith("state_lam") or k.startswith("state_psi") for k in got)
    if not fused:
        assert prog.spec_passes(False)["adj"][-1]          # the last adjoint pass (OBS, readout weights) ran per plan
    if (n, L) == (18, 4):
        assert prog.n_passes == 4
    if (n, L) == (16, 3) and tile is None:
        assert (prog.passes[0][0].t, prog.adj_tile_bits, prog.n_passes) == (14, 13, 2)
    bad = {k: int((got[k] != ref[k]).sum()) for k in ref if not torch.equal(got[k], ref[k])}
    print("mismatching entries:", bad)
    assert not bad


def test_spec_shifted_rows_share_input_samples(cuda):
    """Parameter-shift +pi branches (in_rep > 1: shifted parameter rows read their client's stored sample).  A per-plan
    forward kernel sees in_rep > 1 only for parameters owned by a pass after the first (pass 0, the generation, runs on
    the interpreter), so the plan is the two-pass 16-qubit one; the single-pass 11-qubit plan rides along."""
    for n in (16, 11):
        spec = VQCSpec(n, 3, 3)
        xang, _, _, params = _inputs(spec, 1, 2, cuda)
        outs = []
        for use_spec in (False, True):
            prog = HeaMfmaProgram(spec, cuda, use_spec=use_spec)
            outs.append(prog.shifted_expz(xang, params, with_mean=True).clone())
            if n == 16:
                assert len(prog.shift_owners()[1]) > 0                 # rows that start at pass 1: in_rep = their count
                assert (prog.spec_launches > 0) == use_spec
        assert torch.equal(outs[0], outs[1])


def test_spec_launches_replay_inside_a_graph(cuda):
    """Two local SGD steps of two 16-qubit clients recorded into one graph with the per-plan kernels and replayed
    twice equal the eager interpreter's two steps bitwise."""
    spec = VQCSpec(16, 3, 3)
    K, B, lr = 2, 3, 0.05
    xang, y, w, p0 = _inputs(spec, K, B, cuda)

    def two_steps(prog, params):
        outs = []
        for _ in range(2):
            out = prog.loss_and_grads(xang, y, w, params, spec)
            params.sub_(lr * out["grad"])
            outs.append((out["loss"].clone(), out["grad"].clone()))
        return outs

    ref_p = p0.clone()
    ref = two_steps(HeaMfmaProgram(spec, cuda, use_spec=False), ref_p)
    torch.cuda.synchronize()

    prog = HeaMfmaProgram(spec, cuda, use_spec=True)
    assert prog.spec_active
    params = p0.clone()
    ws = {}
    with prog.private_workspace(ws):
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            two_steps(prog, params)
        torch.cuda.current_stream(cuda).wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            params.copy_(p0)
            got = two_steps(prog, params)
    for _ in range(2):
        gr.replay()
    torch.cuda.synchronize()
    assert prog.spec_launches > 0 and prog.spec_passes() == {"fwd": [False, True], "adj": [True, False]}
    assert torch.equal(params, ref_p)
    for (gl, gg), (rl, rg) in zip(got, ref):
        assert torch.equal(gl, rl) and torch.equal(gg, rg)


def test_spec_selection(cuda, monkeypatch):
    spec = VQCSpec(8, 2, 3)
    monkeypatch.delenv("QFEDX_HEA_SPEC", raising=False)
    monkeypatch.delenv("QFEDX_DEBUG", raising=False)
    assert spec_default() and HeaMfmaProgram(spec, cuda).spec_active      # on by default
    one = HeaMfmaProgram(spec, cuda)                # single pass: per plan only in a step without the fused readout
    assert one.spec_passes(True) == {"fwd": [False], "adj": [False]}
    assert one.spec_passes(False) == {"fwd": [False], "adj": [True]}
    monkeypatch.setenv("QFEDX_HEA_SPEC", "0")
    assert not HeaMfmaProgram(spec, cuda).spec_active
    monkeypatch.setenv("QFEDX_HEA_SPEC", "1")
    assert HeaMfmaProgram(spec, cuda).spec_active
    monkeypatch.setenv("QFEDX_DEBUG", "1")        # the device checks validate records the per-plan build never reads
    assert not spec_default()
