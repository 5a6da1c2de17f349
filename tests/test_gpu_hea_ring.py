"""GPU tests of ring-entangler VQCs on the MFMA statevector engine: ``HeaMfmaProgram`` on ring plans
(``hea_plan.build_plan(ring=True)``) against the float64 dense oracle, the tile-exact emulator (bf16), its own other
launch routes (bitwise), the fp32 VALU engine, and through the public config path.

The pass kernels are table driven and run ring plans unchanged; these tests are what shows it.  fp16 tolerances against
float64 are those of the chain tests at the same (n, tile): <Z> 7.5e-4 and gradient 5e-4 x max(1, |g|max)
(tests/test_gpu_hea.py, tests/test_gpu_hea_amp.py); profiles/hea_ring_err_table.txt holds the measured errors.
"""
import numpy as np
import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_plan as hp
from qfedx_amd.ops.engine import VQCEngine
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
from qfedx_amd.ops.statevec_torch import TorchProgram, slot_grads

pytestmark = pytest.mark.gpu

BOUND_Z, BOUND_G = 7.5e-4, 5e-4


def _dense(spec, params, wread, xang):
    """float64 dense oracle from feature angles xang [K, B, n]."""
    ops, coef = spec.program()
    prog = TorchProgram(ops, coef, spec.n_qubits, dtype=torch.complex128)
    K, B = wread.shape[:2]
    P = spec.n_theta
    rows = torch.cat([params[:, None, :P].double().expand(K, B, P), xang.double()], -1).reshape(K * B, -1)
    psi = prog.run(rows)
    ez = prog.expz(psi, spec.readout).reshape(K, B, -1)
    g = prog.adjoint_grads(rows, psi, wread.reshape(K * B, -1).double(), spec.readout)
    return ez.numpy(), slot_grads(g, prog.ops, prog.coef, rows.shape[1])[:, :P].reshape(K, B, P).sum(1).numpy()


def _inputs(spec, K, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(K, B, spec.n_qubits, generator=g) * 3.0
    params = torch.randn(K, spec.n_params, generator=g)
    wr = torch.randn(K, B, spec.n_classes, generator=g) / B
    return x, params, wr


# ------------------------------------------------------------------------------------------ numerics against float64
@pytest.mark.parametrize("n,L,tile,feat,readout,K,B", [
    (8, 2, 14, "ry", None, 2, 3),                     # one pass, one tile: the wrap vector {7, 0, 1} in a whole-state tile
    (10, 3, 8, "ry", [0, 5, 9], 2, 3),                # three passes, strided tiles, 4 tiles per sample, dense row masks
    (12, 2, 10, "rx", None, 2, 3),                    # two passes, the rx feature map
    (16, 3, 14, "ry", None, 1, 2)])                   # the production plan with the default adjoint tiling
def test_hea_ring_vjp_matches_dense(cuda, n, L, tile, feat, readout, K, B):
    spec = VQCSpec(n, L, 3, feature_map=feat, entangler="ring", readout=readout)
    prog = HeaMfmaProgram(spec, cuda, tile_bits=tile)
    assert prog.ring and prog.plan.ring and prog.adj_plan.ring and prog.grad_cover_exact
    assert prog.n_passes == {8: 1, 10: 3, 12: 2, 16: 3}[n]
    if n == 10:
        assert prog.plan.t == 8 and any(p.lo > p.c for p in prog.plan.passes)      # a strided tile
        assert sum(1 for p in prog.plan.passes if p.l1) >= 2                        # layer-1 groups split over passes
    if n == 16:                                        # both plans run the same groups in the same passes
        sig = lambda pl: [sorted((g.slot, g.layer, tuple(g.qubits)) for g in p.groups) for p in pl.passes]
        assert sig(prog.plan) == sig(prog.adj_plan) and prog.plan.t == 14
    x, params, wr = _inputs(spec, K, B, seed=n)
    ez_ref, g_ref = _dense(spec, params, wr, x)
    z, g = prog.vjp(x.to(cuda), params[:, : spec.n_theta].to(cuda), wr.to(cuda))
    torch.cuda.synchronize()
    scale = max(1.0, float(np.abs(g_ref).max()))
    err_z = float(np.abs(z.cpu().reshape(K, B, -1).numpy() - ez_ref).max())
    err_g = float(np.abs(g.cpu().numpy() - g_ref).max())
    print(f"HEA_RING_ERR n={n} L={L} tile={tile} feature={feat} adj_tile={prog.adj_tile_bits} err_z={err_z:.3e} "
          f"err_g={err_g:.3e} gmax={scale:.3f}")
    assert err_z <= BOUND_Z, (err_z, BOUND_Z)
    assert err_g <= BOUND_G * scale, (err_g, BOUND_G * scale)


def test_hea_ring_vjp_bf16_matches_emulator(cuda):
    """bf16 storage at 10q x 3L, tile 8: the GPU's error against the float64 oracle within 3x the error of the
    tile-exact emulator with bf16 rounding after every op (+ 5e-4: the bound of test_hea_amp_vjp_bf16_matches_emulator)."""
    spec = VQCSpec(10, 3, 3, entangler="ring", readout=[0, 5, 9])
    prog = HeaMfmaProgram(spec, cuda, tile_bits=8, storage="bf16")
    K, B = 2, 3
    x, params, wr = _inputs(spec, K, B, seed=4)
    ez_ref, g_ref = _dense(spec, params, wr, x)
    ez_e, g_e = hp.emulate(prog.plan, x.double().numpy(), params.double().numpy(), wr.double().numpy(), storage="bf16")
    z, g = prog.vjp(x.to(cuda), params[:, : spec.n_theta].to(cuda), wr.to(cuda))
    torch.cuda.synchronize()
    ez_err, g_err = np.abs(ez_e - ez_ref).max(), np.abs(g_e - g_ref).max()
    err_z = np.abs(z.cpu().reshape(K, B, -1).numpy() - ez_ref).max()
    err_g = np.abs(g.cpu().numpy() - g_ref).max()
    print(f"HEA_RING_ERR_BF16 err_z={err_z:.3e} (emulator {ez_err:.3e}) err_g={err_g:.3e} (emulator {g_err:.3e})")
    assert err_z <= 3 * ez_err + 5e-4, (err_z, ez_err)
    assert err_g <= 3 * g_err + 5e-4, (err_g, g_err)


# ------------------------------------------------------------------------------------------ bitwise routes
SHAPES = [(10, 3, 8, 2, 3), (16, 3, 14, 1, 2)]        # (n, L, tile, K, B)


def _train_inputs(spec, K, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(K, B, spec.n_qubits, generator=g)
    y = torch.randint(0, spec.n_classes, (K, B), generator=g)
    w = torch.full((K, B), 1.0 / B)
    params = torch.stack([spec.init_params(k) for k in range(K)])
    params[:, : spec.n_theta] += 0.5 * torch.randn(K, spec.n_theta, generator=g)
    return spec.encode_features(x), y, w, params


def _step(cuda, shape, graph=False, **kw):
    n, L, tile, K, B = shape
    spec = VQCSpec(n, L, 3, entangler="ring", readout_scale=2.0)
    xang, y, w, params = (t.to(cuda) for t in _train_inputs(spec, K, B, seed=9))
    prog = HeaMfmaProgram(spec, cuda, tile_bits=tile, use_spec=kw.pop("use_spec", None))
    for k, v in kw.items():
        setattr(prog, k, v)
    if not graph:
        out = prog.loss_and_grads(xang, y, w, params, spec)
    else:
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
        gr.replay()
        gr.replay()
    torch.cuda.synchronize()
    return prog, {k: v.clone() for k, v in out.items()}


def _same(a, b):
    for k in ("loss", "correct", "grad", "expz"):
        assert torch.equal(a[k], b[k]), k


_BASE = {}


def _base(cuda, shape):
    """The per-plan, split-readout step of a shape: computed once, every route below is compared with it."""
    if shape not in _BASE:
        _BASE[shape] = _step(cuda, shape, use_spec=True, split_readout=True)
    return _BASE[shape]


ROUTES = {"interpreter": dict(use_spec=False, split_readout=True),       # per-plan kernels against the interpreter
          "fused_readout": dict(split_readout=False),                    # fused against split readout
          "second_run": dict(use_spec=True, split_readout=True),         # two runs of the same step
          "captured": dict(graph=True, use_spec=True, split_readout=True),   # a hipGraph, replayed twice, against eager
          "obs_op": dict(use_spec=True, split_readout=True)}             # lambda seeded by the observable op, not the load


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("shape", SHAPES, ids=["10q-tile8", "16q-tile14"])
def test_hea_ring_launch_routes_are_bitwise(cuda, monkeypatch, shape, route):
    S = shape[3] * shape[4]
    ps, base = _base(cuda, shape)
    sp = ps.spec_passes(samples=S)
    assert all(sp["adj"]) and all(sp["fwd"][1:]) and ps.spec_launches > 0 and ps.obs_at_load
    assert ps.readout_mode(S) == "split"
    if route == "obs_op":
        monkeypatch.setenv("QFEDX_HEA_OBS_LOAD", "0")
    prog, out = _step(cuda, shape, **ROUTES[route])
    if route == "interpreter":
        assert prog.spec_launches == 0 and prog.interp_launches > 0
    if route == "fused_readout":
        assert prog.readout_mode(S) == "fused"
    if route == "obs_op":
        assert not prog.obs_at_load
    _same(base, out)


def test_hea_ring_adjoint_tilings_agree(cuda, monkeypatch):
    """16q x 3L: the forward on the 2^13 plan's groups with a 2^13 adjoint, and the native 2^14 groups with a 2^14
    adjoint (QFEDX_HEA_RING_ADJ), are two plans of one circuit: both within the fp16 bounds of the float64 oracle."""
    spec = VQCSpec(16, 3, 3, entangler="ring")
    K, B = 1, 2
    x, params, wr = _inputs(spec, K, B, seed=21)
    ez_ref, g_ref = _dense(spec, params, wr, x)
    scale = max(1.0, float(np.abs(g_ref).max()))
    tiles = {}
    for knob in ("13", "14"):
        monkeypatch.setenv("QFEDX_HEA_RING_ADJ", knob)
        prog = HeaMfmaProgram(spec, cuda)
        tiles[knob] = (prog.adj_tile_bits, prog.plan.n_slots)
        z, g = prog.vjp(x.to(cuda), params[:, : spec.n_theta].to(cuda), wr.to(cuda))
        torch.cuda.synchronize()
        assert np.abs(z.cpu().reshape(K, B, -1).numpy() - ez_ref).max() <= BOUND_Z
        assert np.abs(g.cpu().numpy() - g_ref).max() <= BOUND_G * scale
    assert tiles["13"][0] == 13 and tiles["14"][0] == 14 and tiles["14"][1] <= tiles["13"][1]


def test_hea_ring_captured_round_bitwise_eager(cuda, monkeypatch):
    """Two 3-step rounds through VQCClientTrainer (unequal shards: clients go inactive), captured against eager."""
    from tests.test_fl import small_cfg
    from qfedx_amd.data.datasets import build_federated_data
    from qfedx_amd.fl.adapters import make_adapter
    from qfedx_amd.fl.trainer import ShardStore
    monkeypatch.setenv("QFEDX_HEA_TILE", "8")
    dev = torch.device("cuda", 0)
    cfg = small_cfg(n_qubits=10, n_layers=3, num_clients=4, samples_per_client=24, batch_size=8, local_epochs=1,
                    device="cuda", backend="hip", entangler="ring", state_dtype="mfma")
    data = build_federated_data(cfg, clients=list(range(4)))
    ad = make_adapter(cfg, dev, "hip")
    assert isinstance(ad.engine.hip, HeaMfmaProgram) and ad.engine.hip.ring and ad.engine.hip.plan.t == 8
    sizes = [24, 9, 17, 24]
    store = ShardStore([(X[:m], y[:m]) for (X, y), m in zip(data.clients, sizes)], data.client_ids, dev)
    theta = ad.init_params(cfg.train.seed).to(dev)
    tr = ad.trainer
    outs = {}
    for graphs in (True, False):
        tr.graphs = graphs
        outs[graphs] = []
        for r in range(2):
            rec = tr.run_round(store, [0, 1, 2, 3], theta, r)
            outs[graphs].append((rec["params"][:4].clone(), rec["loss"][:, :4].clone(), rec["correct"][:, :4].clone()))
    for (pg, lg, cg), (pe, le, ce) in zip(outs[True], outs[False]):
        assert lg.shape[0] == 3
        assert torch.equal(pg, pe) and torch.equal(lg, le) and torch.equal(cg, ce)
    assert not torch.equal(outs[True][0][0][0], theta.float())        # the round trained


# ------------------------------------------------------------------------------------------ against the VALU engine
@pytest.mark.parametrize("n,L,tile", [(10, 3, 8), (16, 3, 14)])
def test_hea_ring_train_step_matches_valu_engine(cuda, monkeypatch, n, L, tile):
    """Loss, a / b and theta gradients and hits of a step against the fp32 VALU engine on the same ring spec (bounds
    of test_hea_amp_train_step_matches_valu_engine)."""
    monkeypatch.setenv("QFEDX_HEA_TILE", str(tile))
    spec = VQCSpec(n, L, 3, entangler="ring", readout_scale=2.0)
    K, B = 2, 3
    xang, y, w, params = (t.to(cuda) for t in _train_inputs(spec, K, B))
    ref = VQCEngine(spec, cuda, "hip").loss_and_grads(xang, y, w, params)
    mf = VQCEngine(spec, cuda, "hip", "mfma")
    assert isinstance(mf.hip, HeaMfmaProgram) and mf.hip.ring and mf.hip.plan.t == min(tile, n)
    out = mf.loss_and_grads(xang, y, w, params)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out["loss"].cpu().numpy(), ref["loss"].cpu().numpy(), atol=2e-3)
    np.testing.assert_allclose(out["grad"].cpu().numpy(), ref["grad"].cpu().numpy(), atol=2e-3)
    np.testing.assert_allclose(out["correct"].cpu().numpy(), ref["correct"].cpu().numpy(), atol=1.0)


def test_hea_ring_param_shift_matches_adjoint(cuda):
    """8q x 2L: method="param_shift" (no shots) runs a ring program's shifted circuits as parameter rows of expz
    (prefix reuse stays chain-only); against the adjoint gradient within the bound of
    test_hea_amp_param_shift_matches_adjoint."""
    spec = VQCSpec(8, 2, 3, entangler="ring", readout_scale=2.0)
    K, B = 2, 3
    xang, y, w, params = (t.to(cuda) for t in _train_inputs(spec, K, B, seed=5))
    eng = VQCEngine(spec, cuda, "hip", "mfma")
    adj = eng.loss_and_grads(xang, y, w, params, "adjoint")["grad"]
    ps = eng.loss_and_grads(xang, y, w, params, "param_shift")["grad"]
    torch.cuda.synchronize()
    scale = max(1.0, float(adj.abs().max()))
    np.testing.assert_allclose(ps.cpu().numpy(), adj.cpu().numpy(), atol=4e-3 * scale)
    with pytest.raises(ValueError, match="chain-only"):
        eng.hip.param_shift(xang, params, torch.zeros(K, B, 3, device=cuda))


# ------------------------------------------------------------------------------------------ public config path
def test_hea_ring_federated_run_matches_fp32(cuda):
    """Three federated rounds (plain SGD: Adam's normalised steps would amplify last-bit gradient differences of
    near-zero entries) of a 10-qubit ring config with state_dtype=mfma against fp32: per-round training losses within
    the train-step bound."""
    from tests.test_fl import small_cfg
    from qfedx_amd.api import run_experiment
    from qfedx_amd.parallel.dist import init_distributed
    dev = torch.device("cuda", 0)
    kw = dict(num_rounds=3, optimizer="sgd", entangler="ring", n_qubits=10, device="cuda", backend="hip")
    outs = {sd: run_experiment(small_cfg(state_dtype=sd, **kw), world=init_distributed(dev), device=dev, backend="hip")
            for sd in ("mfma", "fp32")}
    assert len(outs["mfma"]["history"]) == 3
    for a, b in zip(outs["mfma"]["history"], outs["fp32"]["history"]):
        assert np.isfinite(a["train_loss"]) and abs(a["train_loss"] - b["train_loss"]) <= 2e-3, (a, b)
    assert all(np.isfinite(v) for v in outs["mfma"]["accuracies"]) and len(outs["mfma"]["accuracies"]) >= 2


def test_hea_ring_refusals_through_the_config(cuda):
    """An explicit MFMA state_dtype on a ring spec the engine does not cover fails with the reason; auto stays on the
    fp32 VALU engine."""
    from tests.test_fl import small_cfg
    from qfedx_amd.fl.adapters import make_adapter
    dev = torch.device("cuda", 0)
    base = dict(device="cuda", backend="hip", entangler="ring")
    with pytest.raises(ValueError, match="7 qubits is outside 8..30"):
        make_adapter(small_cfg(n_qubits=7, state_dtype="mfma", **base), dev, "hip")
    with pytest.raises(ValueError, match="9 classes"):
        make_adapter(small_cfg(n_qubits=10, n_classes=9, state_dtype="fp16", **base), dev, "hip")
    with pytest.raises(ValueError, match="refused: gate noise"):
        make_adapter(small_cfg(n_qubits=10, state_dtype="mfma", **base, **{"noise.kind": "depolarizing", "noise.p": 0.01}),
                     dev, "hip")
    with pytest.raises(ValueError, match="refused: gate noise"):
        HeaMfmaProgram(VQCSpec(10, 2, 3, entangler="ring", noisy=True), cuda)
    with pytest.raises(ValueError, match="amplitude features with a ring entangler"):
        make_adapter(small_cfg(n_qubits=10, state_dtype="mfma", feature_map="amplitude", **base), dev, "hip")
    ad = make_adapter(small_cfg(n_qubits=10, state_dtype="auto", **base), dev, "hip")
    assert ad.state_dtype == "fp32" and not isinstance(ad.engine.hip, HeaMfmaProgram)
    ad = make_adapter(small_cfg(n_qubits=10, state_dtype="mfma_bf16", **base), dev, "hip")
    assert isinstance(ad.engine.hip, HeaMfmaProgram) and ad.engine.hip.ring and ad.engine.hip.bf16
