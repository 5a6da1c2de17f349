"""Seeding tile load of the per-plan last adjoint pass (``HeaMfmaProgram.obs_at_load``: lambda = (sum_c +-r_c) psi is
written while the tile is loaded and the pass runs no observable op) against the same pass with the op
(``QFEDX_HEA_OBS_LOAD=0``) and against the interpreter (``use_spec=False``), BITWISE: <Z>, the whole gradient, the
lambda the last pass stores where it stores one, and for training steps loss, hits, readout weights and records.

Shapes, the smallest at which each mechanism exists: 8 qubits - one tile of 256 amplitudes under a 512-thread workgroup
(predicated quads); 14 qubits on 2^13 adjoint tiles - two tiles, so the parity of the tile's fixed bits with the class
masks matters; 16 qubits x 3 layers, 6 samples - the headline plan's strided 2^13 tile (c = 5), two passes, the last
one stores lambda; fp16 and bf16 storage.  Class counts 1, 3 and 8 (8: no sign table).  Every vjp case has random
weights and one all-zero weight row (rho = 1).  Training steps on the split route (128 samples), eager and replayed in
a graph.  Every case asserts from the launch counters that the per-plan last pass ran."""
import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_plan as hp
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram

pytestmark = pytest.mark.gpu

MODES = ("interp", "knob0", "knob1")


@pytest.fixture(scope="module", autouse=True)
def _tmp_cache(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("QFEDX_JIT_CACHE", str(tmp_path_factory.mktemp("hea_obs_load_cache")))
    for name in ("QFEDX_HEA_SPLIT_RO", "QFEDX_HEA_SPEC", "QFEDX_DEBUG", "QFEDX_HEA_OBS_LOAD", "QFEDX_HEA_ADJ_TILE",
                 "QFEDX_HEA_TILE"):
        mp.delenv(name, raising=False)
    yield
    mp.undo()


def _spec(n, L, C):
    if C == 1:
        # (VQCSpec wants two classes for its cross entropy; vjp needs none of it: one readout qubit, one class kernel)
        spec = VQCSpec(n, L, 2)
        spec.n_classes, spec.readout = 1, [0]
        return spec
    return VQCSpec(n, L, C, readout_scale=2.0) if C != 3 else VQCSpec(n, L, 3)


def _program(spec, dev, mode, storage="fp16", tile_bits=None):
    mp = pytest.MonkeyPatch()
    try:
        if mode != "interp":
            mp.setenv("QFEDX_HEA_OBS_LOAD", mode[-1])
        prog = HeaMfmaProgram(spec, dev, tile_bits=tile_bits, storage=storage, use_spec=mode != "interp")
    finally:
        mp.undo()
    if mode == "interp":
        assert not prog.spec_active
    else:
        assert prog.obs_at_load is (mode == "knob1") and prog.spec_adj[-1] >= 0
        a, _ = prog._host_progs[-1][1]
        assert int(a[0, hp.W_CODE]) == hp.OP_OBS
    return prog


def _check_launches(prog, mode, steps, samples=None):
    """Per plan: every pass but the generating forward pass, the last adjoint pass among them."""
    if mode == "interp":
        assert prog.spec_launches == 0 and prog.interp_launches > 0
        return
    sp = prog.spec_passes(fused_readout=False) if samples is None else prog.spec_passes(samples=samples)
    assert sp["adj"][-1] and sp["fwd"][0] is False
    n_spec = sum(sp["fwd"]) + sum(sp["adj"])
    assert prog.spec_launches == steps * n_spec
    assert prog.interp_launches == steps * (len(sp["fwd"]) + len(sp["adj"]) - n_spec)


def _mismatches(got, ref):
    assert set(got) == set(ref)
    return {k: int((got[k] != ref[k]).sum()) for k in ref if not torch.equal(got[k], ref[k])}


# name: (qubits, layers, classes, storage, forward tile bits, clients, batch)
VJP = {
    "8q2L_C1": (8, 2, 1, "fp16", None, 2, 3),
    "8q2L_C3": (8, 2, 3, "fp16", None, 2, 3),
    "8q2L_C8": (8, 2, 8, "fp16", None, 2, 3),
    "14q2L_t13_C3": (14, 2, 3, "fp16", 13, 2, 2),
    "14q2L_t13_C8": (14, 2, 8, "fp16", 13, 2, 2),
    "16q3L_C3": (16, 3, 3, "fp16", None, 2, 3),
    "16q3L_bf16": (16, 3, 3, "bf16", None, 2, 3),
}


def _vjp(name, dev, mode):
    n, L, C, storage, tile, K, B = VJP[name]
    spec = _spec(n, L, C)
    g = torch.Generator().manual_seed(11)
    xang = spec.encode_features(torch.rand(K, B, n, generator=g)).to(dev)
    theta = (0.1 * torch.randn(K, spec.n_theta, generator=g) + 0.4 * torch.rand(K, spec.n_theta, generator=g)).to(dev)
    w = torch.randn(K * B, C, generator=g)
    w[1] = 0.0                                             # a weight row of zeros: rho = 1, lambda = 0
    prog = _program(spec, dev, mode, storage, tile)
    z, grad = prog.vjp(xang, theta, w.to(dev))
    torch.cuda.synchronize()
    _check_launches(prog, mode, 1)
    res = {"expz": z.clone(), "grad": grad.clone()}
    S = K * B
    for nm, t in prog._ws.items():
        if nm.startswith("lam"):
            res["state_" + nm] = t[: S << n].clone()
    return res, prog


@pytest.mark.parametrize("name", list(VJP))
def test_vjp_is_bitwise_with_and_without_the_seeding_load(cuda, name):
    n, L, C, storage, tile, K, B = VJP[name]
    out = {m: _vjp(name, cuda, m) for m in MODES}
    prog = out["knob1"][1]
    t_last = prog.passes[-1][3].t
    if name.startswith("8q"):
        assert (prog.n_passes, t_last) == (1, 8)           # 64 quads under 512 threads
    if name.startswith("14q"):
        assert (t_last, 1 << (n - t_last)) == (13, 2)      # two tiles per sample
    if name.startswith("16q"):
        p = prog.passes[-1][3]
        assert (prog.n_passes, p.t, p.c) == (2, 13, 5) and p.lo > p.c      # strided tile
        assert any(k.startswith("state_lam") for k in out["knob1"][0])    # the last pass stores lambda
    assert torch.isfinite(out["knob1"][0]["grad"]).all() and out["knob1"][0]["grad"].abs().max() > 0
    for ref in ("knob0", "interp"):
        bad = _mismatches(out["knob1"][0], out[ref][0])
        print(name, "knob1 vs", ref, "mismatching entries:", bad)
        assert not bad


# ------------------------------------------------------------------------------------------------ training steps
def _train_inputs(spec, K, B, dev):
    g = torch.Generator().manual_seed(5)
    xang = spec.encode_features(torch.rand(K, B, spec.n_qubits, generator=g)).to(dev)
    y = torch.randint(0, spec.n_classes, (K, B), generator=g).to(dev)
    w = torch.rand(K, B, generator=g) / B
    w[K // 2, B // 2] = 0.0                                # a weight-0 sample: its readout weights are all zero
    params = torch.stack([spec.init_params(k) for k in range(K)])
    params = (params + 0.3 * torch.randn(params.shape, generator=g)).to(dev)
    return xang, y, w.to(dev), params


def _two_steps(prog, spec, xang, y, w, params, lr=0.05):
    outs = []
    for _ in range(2):
        out = prog.loss_and_grads(xang, y, w, params, spec)
        params.sub_(lr * out["grad"])
        outs.append({k: out[k].clone() for k in ("loss", "correct", "grad", "expz")})
    return outs


@pytest.fixture(scope="module")
def train_ref(cuda):
    """Two SGD steps of 4 clients x 32 samples (128: the split route) at 10 qubits, per mode, eager."""
    spec = VQCSpec(10, 3, 3)
    K, B = 4, 32
    xang, y, w, p0 = _train_inputs(spec, K, B, cuda)
    res = {}
    for mode in MODES:
        prog = _program(spec, cuda, mode)
        params = p0.clone()
        outs = _two_steps(prog, spec, xang, y, w, params)
        torch.cuda.synchronize()
        if mode != "interp":
            assert prog.readout_mode(K * B) == "split"
        _check_launches(prog, mode, 2, samples=K * B)
        S = K * B
        last = {"params": params.clone(), "wread": prog._ws["wread"][: S * 3].clone(),
                "rorec": prog._ws["rorec"][: S * 8].clone()}
        res[mode] = (outs, last)
    return spec, (xang, y, w, p0), res


def test_split_training_steps_are_bitwise(train_ref):
    _, _, res = train_ref
    outs1, last1 = res["knob1"]
    assert (last1["wread"].view(-1, 3).abs().amax(1) == 0).sum() == 1          # the weight-0 sample
    for ref in ("knob0", "interp"):
        outs, last = res[ref]
        for a, b in zip(outs1, outs):
            assert not _mismatches(a, b)
        assert not _mismatches(last1, last)


def test_split_training_steps_replay_inside_a_graph(cuda, train_ref):
    spec, (xang, y, w, p0), res = train_ref
    K, B = w.shape
    prog = _program(spec, cuda, "knob1")
    params = p0.clone()
    ws = {}
    with prog.private_workspace(ws):
        side = torch.cuda.Stream(device=cuda)
        side.wait_stream(torch.cuda.current_stream(cuda))
        with torch.cuda.stream(side):
            _two_steps(prog, spec, xang, y, w, params)
        torch.cuda.current_stream(cuda).wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            params.copy_(p0)
            got = _two_steps(prog, spec, xang, y, w, params)
    for _ in range(2):
        gr.replay()
    torch.cuda.synchronize()
    _check_launches(prog, "knob1", 4, samples=K * B)       # the warm-up and the capture: two steps each
    outs, last = res["interp"]
    assert torch.equal(params, last["params"])
    for a, b in zip(got, outs):
        assert not _mismatches(a, b)
