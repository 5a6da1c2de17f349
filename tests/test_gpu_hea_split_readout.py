"""Split-readout training steps of the MFMA engine (``HeaMfmaProgram.readout_mode``: ``hea_readout_rec`` writes every
sample's <Z>, dL/d<Z> and reduction record, and the last adjoint pass runs its per-plan kernel) against the fused steps
(the last adjoint pass computes them, on the interpreter), BITWISE: loss, hits, the whole gradient (theta and readout
parameters), <Z>, the readout weights and records, and every stored pass state.

Shapes: the smallest at which each mechanism exists - one pass that is both first and last, with a partial tile; the
smallest pair-op plan; the headline two-pass plan (2^13 adjoint tiles: 8 workgroups per sample recomputed the fused
readout) in fp16 and bf16; four passes; non-uniform loss weights with a weight-0 sample (the adjoint pass's rho == 0
branch); 8 classes, the maximum.  Every case asserts from the launch counters which kernel ran the last adjoint pass."""
import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _tmp_cache(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("QFEDX_JIT_CACHE", str(tmp_path_factory.mktemp("hea_split_cache")))
    mp.delenv("QFEDX_HEA_SPLIT_RO", raising=False)
    mp.delenv("QFEDX_HEA_SPEC", raising=False)
    mp.delenv("QFEDX_DEBUG", raising=False)
    yield
    mp.undo()


def _inputs(spec, K, B, dev, weights="uniform", seed=5):
    g = torch.Generator().manual_seed(seed)
    n = spec.n_qubits
    xang = spec.encode_features(torch.rand(K, B, n, generator=g)).to(dev)
    y = torch.randint(0, spec.n_classes, (K, B), generator=g).to(dev)
    if weights == "uniform":
        w = torch.full((K, B), 1.0 / B)
    else:
        w = torch.rand(K, B, generator=g) / B
        w[K // 2, B // 2] = 0.0
    params = torch.stack([spec.init_params(k) for k in range(K)])
    params = (params + 0.3 * torch.randn(params.shape, generator=g)).to(dev)
    return xang, y, w.to(dev), params


def _program(spec, dev, split, storage="fp16"):
    prog = HeaMfmaProgram(spec, dev, storage=storage, use_spec=True)
    assert prog.spec_active and prog.spec_adj[-1] >= 0
    prog.split_readout = split
    return prog


def _check_launches(prog, S, split, steps=1):
    """The last adjoint pass ran per plan on the split route and on the interpreter on the fused one; every other
    pass as ``spec_passes`` names it."""
    assert prog.readout_mode(S) == ("split" if split else "fused")
    sp = prog.spec_passes(samples=S)
    assert sp["adj"][-1] == split
    assert sp["fwd"] == prog.spec_passes()["fwd"] and sp["adj"][:-1] == prog.spec_passes()["adj"][:-1]
    assert not prog.spec_passes()["adj"][-1]
    n_spec = sum(sp["fwd"]) + sum(sp["adj"])
    assert prog.spec_launches == steps * n_spec
    assert prog.interp_launches == steps * (len(sp["fwd"]) + len(sp["adj"]) - n_spec)


def _step(spec, dev, K, B, split, storage="fp16", weights="uniform"):
    xang, y, w, params = _inputs(spec, K, B, dev, weights)
    prog = _program(spec, dev, split, storage)
    out = prog.loss_and_grads(xang, y, w, params, spec)
    torch.cuda.synchronize()
    _check_launches(prog, K * B, split)
    res = {k: out[k].clone() for k in ("loss", "correct", "grad", "expz")}
    S = K * B
    for name, t in prog._ws.items():
        if name.startswith(("psi", "lam")):
            res["state_" + name] = t[: S << spec.n_qubits].clone()
    res["wread"] = prog._ws["wread"][: S * spec.n_classes].clone()
    res["rorec"] = prog._ws["rorec"][: S * (2 * spec.n_classes + 2)].clone()
    return res, prog


# name: (qubits, layers, clients, batch, classes, storage, loss weights)
SHAPES = {
    "8q2L": (8, 2, 2, 3, 3, "fp16", "uniform"),          # one pass: the same pass is first and last; partial tile
    "11q3L": (11, 3, 2, 2, 3, "fp16", "uniform"),        # pair ops
    "16q3L": (16, 3, 2, 3, 3, "fp16", "uniform"),        # two passes, 2^13 adjoint tiles
    "16q3L_bf16": (16, 3, 2, 3, 3, "bf16", "uniform"),
    "18q4L": (18, 4, 1, 2, 3, "fp16", "uniform"),        # four passes
    "12q_w0": (12, 3, 5, 7, 4, "fp16", "random"),        # non-uniform weights, one sample of weight 0 (rho == 0)
    "10q_C8": (10, 3, 3, 4, 8, "fp16", "uniform"),       # the class maximum
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_split_step_is_bitwise_the_fused_step(cuda, name):
    n, L, K, B, C, storage, weights = SHAPES[name]
    spec = VQCSpec(n, L, C, readout_scale=2.0) if C != 3 else VQCSpec(n, L, 3)
    ref, _ = _step(spec, cuda, K, B, False, storage, weights)
    got, prog = _step(spec, cuda, K, B, True, storage, weights)
    assert set(got) == set(ref) and any(k.startswith("state_psi") for k in got)
    if name == "8q2L":
        assert prog.n_passes == 1 and prog.spec_launches == 1
    if name.startswith("16q3L"):
        assert (prog.adj_tile_bits, prog.n_passes, prog.tiles_last) == (13, 2, 4)
        assert any(k.startswith("state_lam") for k in got)
    if name == "18q4L":
        assert prog.n_passes == 4
    if name == "12q_w0":
        S, Cn = K * B, spec.n_classes
        assert (got["wread"].view(S, Cn).abs().amax(1) == 0).sum() == 1        # the weight-0 sample: rho == 0
    bad = {k: int((got[k] != ref[k]).sum()) for k in ref if not torch.equal(got[k], ref[k])}
    print("mismatching entries:", bad)
    assert not bad


def test_split_steps_replay_inside_a_graph(cuda):
    """Two local SGD steps of two 16-qubit clients recorded into one graph with the split route forced and replayed
    twice equal the eager fused steps bitwise."""
    spec = VQCSpec(16, 3, 3)
    K, B, lr = 2, 3, 0.05
    xang, y, w, p0 = _inputs(spec, K, B, cuda)

    def two_steps(prog, params):
        outs = []
        for _ in range(2):
            out = prog.loss_and_grads(xang, y, w, params, spec)
            params.sub_(lr * out["grad"])
            outs.append((out["loss"].clone(), out["correct"].clone(), out["grad"].clone(), out["expz"].clone()))
        return outs

    ref_p = p0.clone()
    fused = _program(spec, cuda, False)
    ref = two_steps(fused, ref_p)
    torch.cuda.synchronize()
    _check_launches(fused, K * B, False, steps=2)

    prog = _program(spec, cuda, True)
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
    _check_launches(prog, K * B, True, steps=4)          # the warm-up and the capture: two steps each
    assert {"wread", "rorec", "part"} <= set(ws) and not prog._ws
    assert torch.equal(params, ref_p)
    for g_, r_ in zip(got, ref):
        for a, b in zip(g_, r_):
            assert torch.equal(a, b)


def _adam_steps(spec, dev, split, acts, w, xs, ys, p0):
    from qfedx_amd.fl.optim import BatchedOptimizer
    prog = _program(spec, dev, split)
    p = p0.clone()
    opt = BatchedOptimizer("adam", p.shape, dev, 0.05, backend="hip")
    outs = []
    for s, act in enumerate(acts):
        res = prog.loss_and_grads(xs[s], ys[s], w, p, spec, fused_opt=(opt, act))
        assert res.get("opt_done", False)
        outs.append((res["loss"].clone(), res["correct"].clone(), res["grad"].clone()))
    torch.cuda.synchronize()
    _check_launches(prog, p0.shape[0] * w.shape[1], split, steps=len(acts))
    return p, opt.m.clone(), opt.v.clone(), opt.t.clone(), outs


def _adam_case(dev, K=5, B=8):
    spec = VQCSpec(n_qubits=12, n_layers=2, n_classes=3)
    g = torch.Generator().manual_seed(7)
    xs = [spec.encode_features(torch.rand(K, B, 12, generator=g)).to(dev) for _ in range(3)]
    ys = [torch.randint(0, 3, (K, B), generator=g).to(dev) for _ in range(3)]
    p0 = torch.stack([spec.init_params(k) for k in range(K)]).to(dev)
    return spec, xs, ys, p0


def test_fused_adam_is_bitwise_on_both_routes(cuda):
    """The Adam step in hea_grad_reduce's epilogue (<= 256 reduction blocks; the readout block owns the readout
    parameters) gives bitwise the same parameters, moments and step counters on the split route, over several steps
    with clients that drop out."""
    K, B = 5, 8
    spec, xs, ys, p0 = _adam_case(cuda, K, B)
    w = torch.full((K, B), 1.0 / B, device=cuda)
    acts = [torch.tensor(a, dtype=torch.float32, device=cuda)
            for a in ([1, 1, 1, 1, 1], [1, 0, 1, 1, 0], [0, 0, 1, 1, 0])]
    pa, ma, va, ta, oa = _adam_steps(spec, cuda, False, acts, w, xs, ys, p0)
    pb, mb, vb, tb, ob = _adam_steps(spec, cuda, True, acts, w, xs, ys, p0)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ta, tb)
    assert tb.tolist() == [2, 1, 3, 3, 1] and not torch.equal(pb[0], p0[0])
    for sa, sb in zip(oa, ob):
        for a, b in zip(sa, sb):
            assert torch.equal(a, b)


def test_padded_inactive_client_row_passes_through(cuda):
    """A padding row of a round graph (loss weights 0, never active: trainer.graph_bucket) on the split route: its
    parameters and moments stay untouched, its loss and hits are zero, and the active rows are bitwise the fused
    route's."""
    K, B = 4, 8
    spec, xs, ys, p0 = _adam_case(cuda, K, B)
    w = torch.full((K, B), 1.0 / B, device=cuda)
    w[K - 1] = 0.0
    acts = [torch.tensor([1, 1, 1, 0], dtype=torch.float32, device=cuda)] * 2
    pa, ma, va, ta, oa = _adam_steps(spec, cuda, False, acts, w, xs, ys, p0)
    pb, mb, vb, tb, ob = _adam_steps(spec, cuda, True, acts, w, xs, ys, p0)
    assert torch.equal(pb[K - 1], p0[K - 1]) and not mb[K - 1].any() and not vb[K - 1].any() and tb[K - 1] == 0
    for loss, correct, _ in ob:
        assert loss[K - 1] == 0 and correct[K - 1] == 0
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ta, tb)
    for sa, sb in zip(oa, ob):
        for a, b in zip(sa, sb):
            assert torch.equal(a, b)
