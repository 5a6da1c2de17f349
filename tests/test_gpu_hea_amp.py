"""GPU tests of amplitude-encoded VQCs on the MFMA statevector engine: the staging kernel (csrc/hea_amp.hip) against
its numpy reference, and ``HeaMfmaProgram`` started from staged states against the float64 dense oracle, the tile-exact
emulator, the fp32 VALU engine and its own other launch routes (bitwise).

fp16 tolerances against float64: the angle bounds of tests/test_gpu_hea.py (<Z> 7.5e-4, gradient 5e-4 x max(1, |g|max))
or 3x the error measured per case, whichever is larger, never past that file's loosest fp16 bounds (3e-3 / 4e-3 x
max(1, |g|max)): profiles/hea_amp_err_table.txt holds the measured table.
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

# (n, L, tile) -> (<Z> bound, gradient bound x max(1, |g|max)); see the module docstring.  Measured (<Z>, gradient):
# 8q 1.4e-4 / 2.4e-4, 10q (8 classes) 3.2e-4 / 1.3e-4, 12q 1.6e-4 / 1.1e-4, 15q 1.3e-4 / 9.4e-5: two entries sit above
# the angle bound (3 x 2.4e-4 -> 8e-4 for the 8q gradient, 3 x 3.2e-4 -> 1e-3 for the 10q <Z>), the rest keep it.
BOUNDS = {(8, 1, 14): (7.5e-4, 8e-4), (10, 2, 14): (1e-3, 5e-4), (12, 2, 10): (7.5e-4, 5e-4),
          (15, 2, 14): (7.5e-4, 5e-4)}


def _rows(S, F, seed):
    """Raw feature rows [S, F]: signed Gaussian, image-like (non-negative, mostly zeros), one-hot, all-zero, Gaussian."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, F, generator=g)
    if S > 1:
        x[1] = torch.rand(F, generator=g) * (torch.rand(F, generator=g) < 0.2)
    if S > 2:
        x[2] = 0.0
        x[2, F // 3] = 2.0
    if S > 3:
        x[3] = 0.0
    return x


def _dense(spec, x, params, wread):
    """float64 dense oracle from the raw rows x [K, B, F]."""
    ops, coef = spec.program()
    prog = TorchProgram(ops, coef, spec.n_qubits, dtype=torch.complex128)
    K, B, _ = x.shape
    P = spec.n_theta
    st = spec.initial_states(x.double()).to(torch.complex128).reshape(K * B, -1)
    xz = torch.zeros(K, B, spec.x_width, dtype=torch.float64)
    rows = torch.cat([params[:, None, :P].double().expand(K, B, P), xz], -1).reshape(K * B, -1)
    psi = prog.run(rows, state=st)
    ez = prog.expz(psi, spec.readout).reshape(K, B, -1)
    g = prog.adjoint_grads(rows, psi, wread.reshape(K * B, -1).double(), spec.readout)
    return ez, slot_grads(g, prog.ops, prog.coef, rows.shape[1])[:, :P].reshape(K, B, P).sum(1)


def _inputs(spec, K, B, F, seed=0):
    g = torch.Generator().manual_seed(seed + 100)
    x = _rows(K * B, F, seed)[torch.randperm(K * B, generator=g)].reshape(K, B, F)
    params = torch.randn(K, spec.n_params, generator=g)
    wr = torch.randn(K, B, spec.n_classes, generator=g) / B
    return x, params, wr


def _dummy(spec, x):
    return spec.encode_features(x)


# ------------------------------------------------------------------------------------------ staging kernel
def _ordered(bits):
    """Sign-magnitude 16-bit patterns -> integers ordered like the values they encode."""
    b = bits.astype(np.int64) & 0xFFFF
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def _decode(words, bf16):
    w = words.cpu().numpy().view(np.uint32)
    lo, hi = (w & 0xFFFF).astype(np.uint16), (w >> 16).astype(np.uint16)
    val = (lo.astype(np.uint32) << 16).view(np.float32).astype(np.float64) if bf16 else lo.view(np.float16).astype(np.float64)
    return lo, hi, val


def _ref_bits(ref, bf16):
    if bf16:
        return (ref.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return ref.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n,F,pad", [(8, 256, 0), (10, 784, 0), (10, 784, 3), (13, 8192, 0), (14, 10000, 1),
                                     (15, 1 << 15, 0), (16, 40000, 0)])
def test_amp_stage_matches_reference(cuda, n, F, pad, bf16):
    """Row widths: one 16-byte vector per thread (n <= 12), 2 / 4 / 8 register-resident vectors (13, 14, 15: the
    largest row read once) and the two-read form (16); ``pad``: a strided view whose rows start off 16-byte
    boundaries."""
    from qfedx_amd.ops._ext import ext
    S, N = 5, 1 << n
    x = _rows(S, F, seed=n + pad)
    buf = torch.zeros(S, F + pad)
    buf[:, :F] = x
    xc = buf.to(cuda)[:, :F]
    assert xc.stride(0) == F + pad
    scale = float(1 << (n // 2))
    psi = torch.full((S * N + 8,), -1, dtype=torch.int32, device=cuda)
    ext().hea_amp_stage(xc, n, psi[: S * N], scale, bf16)
    torch.cuda.synchronize()
    assert (psi[S * N:] == -1).all()                                  # nothing past the last row
    lo, hi, val = _decode(psi[: S * N].view(S, N), bf16)
    ref = hp.amp_stage_ref(x.numpy(), n, "bf16" if bf16 else "fp16")
    assert not hi.any()                                               # im halves exactly 0
    assert np.abs(_ordered(lo) - _ordered(_ref_bits(ref, bf16))).max() <= 1   # one unit in the last place
    assert not val[[0, 1, 2, 4], F:].any()                            # padded positions exactly 0
    assert np.array_equal(val[3], ref[3]) and np.all(val[3] == val[3, 0]) and val[3, 0] > 0   # zero row: uniform
    assert val[2, F // 3] == scale and np.count_nonzero(val[2]) == 1  # one-hot: exactly 2^(n // 2)
    # a row stages to the same bits alone, inside the batch, and from a contiguous (aligned) copy
    whole = torch.empty(S * N, dtype=torch.int32, device=cuda)
    ext().hea_amp_stage(xc.contiguous(), n, whole, scale, bf16)
    assert torch.equal(whole, psi[: S * N])
    for s in range(S):
        one = torch.empty(N, dtype=torch.int32, device=cuda)
        ext().hea_amp_stage(xc[s:s + 1], n, one, scale, bf16)
        assert torch.equal(one, psi[s * N:(s + 1) * N]), s


def test_amp_stage_validates_its_arguments(cuda):
    from qfedx_amd.ops._ext import ext
    st = ext().hea_amp_stage
    x = torch.randn(2, 300, device=cuda)
    psi = torch.empty(2 << 8, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError, match="F > 2\\^n"):
        st(x, 8, psi, 16.0, False)
    x = x[:, :256]
    with pytest.raises(ValueError, match="psi too small"):
        st(x, 8, psi[:-1], 16.0, False)
    with pytest.raises(ValueError, match="float32"):
        st(x.double(), 8, psi, 16.0, False)
    with pytest.raises(ValueError, match="inner stride"):
        st(torch.randn(256, 2, device=cuda).t(), 8, psi, 16.0, False)
    with pytest.raises(ValueError, match="int32"):
        st(x, 8, psi.float(), 16.0, False)
    with pytest.raises(ValueError, match="power of two"):
        st(x, 8, psi, 12.0, False)
    with pytest.raises(ValueError, match="aligned"):
        st(x, 8, torch.empty((2 << 8) + 1, dtype=torch.int32, device=cuda)[1:], 16.0, False)
    with pytest.raises(ValueError, match="qubits"):
        st(x[:, :100], 7, psi, 8.0, False)
    st(x, 8, psi, 16.0, False)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ engine numerics
@pytest.mark.parametrize("n,L,tile,C,F", [(8, 1, 14, 3, 256), (10, 2, 14, 8, 784), (12, 2, 10, 3, 4096),
                                          (15, 2, 14, 3, 1 << 15)])
def test_hea_amp_vjp_matches_dense(cuda, n, L, tile, C, F):
    """<Z> and the VJP gradient from raw rows (one image-like, one one-hot) against the float64 dense oracle."""
    spec = VQCSpec(n, L, C, feature_map="amplitude")
    prog = HeaMfmaProgram(spec, cuda, tile_bits=tile)
    assert prog.amplitude and prog.grad_cover_exact and all(not p.l1 for p in prog.plan.passes)
    K, B = 2, 3
    x, params, wr = _inputs(spec, K, B, F, seed=n)
    ez_ref, g_ref = _dense(spec, x, params, wr)
    z, g = prog.vjp(_dummy(spec, x).to(cuda), params[:, : spec.n_theta].to(cuda), wr.to(cuda), init=x.to(cuda))
    torch.cuda.synchronize()
    scale = max(1.0, float(g_ref.abs().max()))
    err_z = float(np.abs(z.cpu().reshape(K, B, -1).numpy() - ez_ref.numpy()).max())
    err_g = float(np.abs(g.cpu().numpy() - g_ref.numpy()).max())
    print(f"HEA_AMP_ERR n={n} L={L} tile={tile} C={C} F={F} err_z={err_z:.3e} err_g={err_g:.3e} gmax={scale:.3f}")
    bz, bg = BOUNDS[(n, L, tile)]
    assert bz <= 3e-3 and bg <= 4e-3
    assert err_z <= bz, (err_z, bz)
    assert err_g <= bg * scale, (err_g, bg * scale)
    z2 = prog.expz(_dummy(spec, x).to(cuda), params[:, : spec.n_theta].to(cuda), init=x.to(cuda))
    np.testing.assert_allclose(z2.cpu().numpy(), z.cpu().reshape(K, B, -1).numpy(), atol=1e-6)


def test_hea_amp_vjp_bf16_matches_emulator(cuda):
    """bf16 storage at 10q x 2L: the GPU's error against the float64 oracle within 3x the error of the tile-exact
    emulator started from the same rows and rounded as the staging kernel rounds (+ 5e-4: the bound of
    test_hea_vjp_matches_dense_bf16)."""
    n, L = 10, 2
    spec = VQCSpec(n, L, 3, feature_map="amplitude")
    prog = HeaMfmaProgram(spec, cuda, storage="bf16")
    K, B = 2, 3
    x, params, wr = _inputs(spec, K, B, 784, seed=4)
    ez_ref, g_ref = _dense(spec, x, params, wr)
    st = spec.initial_states(x.double()).to(torch.complex128).numpy()
    ez_e, g_e = hp.emulate(prog.plan, None, params.double().numpy(), wr.double().numpy(), storage="bf16", init=st)
    z, g = prog.vjp(_dummy(spec, x).to(cuda), params[:, : spec.n_theta].to(cuda), wr.to(cuda), init=x.to(cuda))
    torch.cuda.synchronize()
    ez_err, g_err = np.abs(ez_e - ez_ref.numpy()).max(), np.abs(g_e - g_ref.numpy()).max()
    err_z = np.abs(z.cpu().reshape(K, B, -1).numpy() - ez_ref.numpy()).max()
    err_g = np.abs(g.cpu().numpy() - g_ref.numpy()).max()
    print(f"HEA_AMP_ERR_BF16 err_z={err_z:.3e} (emulator {ez_err:.3e}) err_g={err_g:.3e} (emulator {g_err:.3e})")
    assert err_z <= 3 * ez_err + 5e-4, (err_z, ez_err)
    assert err_g <= 3 * g_err + 5e-4, (err_g, g_err)


def _train_inputs(spec, K, B, F, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = _rows(K * B, F, seed).reshape(K, B, F)
    y = torch.randint(0, spec.n_classes, (K, B), generator=g)
    w = torch.full((K, B), 1.0 / B)
    params = torch.stack([spec.init_params(k) for k in range(K)])
    params[:, : spec.n_theta] += 0.5 * torch.randn(K, spec.n_theta, generator=g)
    return x, y, w, params


@pytest.mark.parametrize("n,L,tile,F", [(10, 2, 14, 784), (12, 2, 10, 4096)])
def test_hea_amp_train_step_matches_valu_engine(cuda, monkeypatch, n, L, tile, F):
    """Loss, a / b and theta gradients of a step against the fp32 VALU engine from the same raw rows (bounds of
    test_hea_train_step_matches_valu_engine)."""
    monkeypatch.setenv("QFEDX_HEA_TILE", str(tile))
    spec = VQCSpec(n, L, 3, feature_map="amplitude", readout_scale=2.0)
    K, B = 2, 3
    x, y, w, params = _train_inputs(spec, K, B, F)
    xc, dm = x.to(cuda), _dummy(spec, x).to(cuda)
    ref = VQCEngine(spec, cuda, "hip").loss_and_grads(dm, y.to(cuda), w.to(cuda), params.to(cuda), init=xc)
    mf = VQCEngine(spec, cuda, "hip", "mfma")
    assert isinstance(mf.hip, HeaMfmaProgram) and mf.hip.plan.t == min(tile, n)
    out = mf.loss_and_grads(dm, y.to(cuda), w.to(cuda), params.to(cuda), init=xc)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out["loss"].cpu().numpy(), ref["loss"].cpu().numpy(), atol=2e-3)
    np.testing.assert_allclose(out["grad"].cpu().numpy(), ref["grad"].cpu().numpy(), atol=2e-3)
    np.testing.assert_allclose(out["correct"].cpu().numpy(), ref["correct"].cpu().numpy(), atol=1.0)


# ------------------------------------------------------------------------------------------ bitwise routes (12q, tile 10)
def _step12(cuda, **kw):
    spec = VQCSpec(12, 2, 3, feature_map="amplitude", readout_scale=2.0)
    K, B = 2, 3
    x, y, w, params = _train_inputs(spec, K, B, 4096, seed=9)
    prog = HeaMfmaProgram(spec, cuda, tile_bits=10, use_spec=kw.pop("use_spec", None))
    for k, v in kw.items():
        setattr(prog, k, v)
    out = prog.loss_and_grads(_dummy(spec, x).to(cuda), y.to(cuda), w.to(cuda), params.to(cuda), spec, init=x.to(cuda))
    torch.cuda.synchronize()
    return prog, {k: v.clone() for k, v in out.items()}


def _same(a, b):
    for k in ("loss", "correct", "grad", "expz"):
        assert torch.equal(a[k], b[k]), k


def test_hea_amp_per_plan_kernels_bitwise_interpreter(cuda):
    """Forward pass 0 of an amplitude program has no generation block: it runs per plan like every other pass."""
    ps, spec_out = _step12(cuda, use_spec=True, split_readout=True)
    pi, interp_out = _step12(cuda, use_spec=False, split_readout=True)
    sp = ps.spec_passes(samples=6)
    assert sp["fwd"][0] is True and all(sp["fwd"]) and all(sp["adj"])
    assert ps.spec_cfg(0, False)[6] == 0
    assert ps.spec_launches > 0 and ps.interp_launches == 0 and pi.spec_launches == 0
    _same(spec_out, interp_out)


def test_hea_amp_fused_readout_bitwise_split(cuda):
    pf, fused = _step12(cuda, split_readout=False)
    ps, split = _step12(cuda, split_readout=True)
    assert pf.readout_mode(6) == "fused" and ps.readout_mode(6) == "split"
    _same(fused, split)


def test_hea_amp_obs_at_load_bitwise(cuda, monkeypatch):
    outs = []
    for knob in ("0", "1"):
        monkeypatch.setenv("QFEDX_HEA_OBS_LOAD", knob)
        prog, out = _step12(cuda, split_readout=True)
        assert prog.obs_at_load == (knob == "1")
        outs.append(out)
    _same(*outs)


def test_hea_amp_expz_chunks_bitwise(cuda):
    """A budget of one client's two live states stages and evaluates client by client."""
    spec = VQCSpec(12, 2, 3, feature_map="amplitude")
    K, B = 3, 3
    x, params, _ = _inputs(spec, K, B, 4096, seed=6)
    args = (_dummy(spec, x).to(cuda), params[:, : spec.n_theta].to(cuda))
    whole = HeaMfmaProgram(spec, cuda, tile_bits=10).expz(*args, init=x.to(cuda))
    small = HeaMfmaProgram(spec, cuda, tile_bits=10)
    small._ps_budget = 2 * B * (1 << 12) * 4
    staged = []
    real = small._stage
    small._stage = lambda init, k, b, tag="": staged.append(k) or real(init, k, b, tag)
    part = small.expz(*args, init=x.to(cuda))
    torch.cuda.synchronize()
    assert staged == [1, 1, 1]
    assert torch.equal(whole, part)


def test_hea_amp_captured_round_bitwise_eager(cuda, monkeypatch):
    """A 3-step round through VQCClientTrainer (unequal shards: clients go inactive), captured against eager: the
    staged input buffer belongs to the captured round's workspace."""
    from tests.test_fl import small_cfg
    from qfedx_amd.data.datasets import build_federated_data
    from qfedx_amd.fl.adapters import make_adapter
    from qfedx_amd.fl.trainer import ShardStore
    monkeypatch.setenv("QFEDX_HEA_TILE", "10")
    dev = torch.device("cuda", 0)
    cfg = small_cfg(n_qubits=12, n_layers=2, num_clients=4, samples_per_client=24, batch_size=8, local_epochs=1,
                    device="cuda", backend="hip", feature_map="amplitude", state_dtype="mfma")
    data = build_federated_data(cfg, clients=list(range(4)))
    ad = make_adapter(cfg, dev, "hip")
    assert isinstance(ad.engine.hip, HeaMfmaProgram) and ad.engine.hip.amplitude and ad.engine.hip.plan.t == 10
    sizes = [24, 9, 17, 24]                          # clients run 3, 2, 3 and 3 steps, some on short last batches
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


# ------------------------------------------------------------------------------------------ parameter shift, runs, refusals
def test_hea_amp_param_shift_matches_adjoint(cuda):
    """8q x 1L: method="param_shift" (no shots) runs the shifted circuits as parameter rows of expz(init=...); against
    the adjoint gradient within the bound test_param_shift_exact_matches_adjoint_oracle uses."""
    spec = VQCSpec(8, 1, 3, feature_map="amplitude", readout_scale=2.0)
    K, B = 2, 3
    x, y, w, params = _train_inputs(spec, K, B, 200, seed=5)
    eng = VQCEngine(spec, cuda, "hip", "mfma")
    args = (_dummy(spec, x).to(cuda), y.to(cuda), w.to(cuda), params.to(cuda))
    adj = eng.loss_and_grads(*args, "adjoint", init=x.to(cuda))["grad"]
    ps = eng.loss_and_grads(*args, "param_shift", init=x.to(cuda))["grad"]
    torch.cuda.synchronize()
    scale = max(1.0, float(adj.abs().max()))
    np.testing.assert_allclose(ps.cpu().numpy(), adj.cpu().numpy(), atol=4e-3 * scale)
    with pytest.raises(ValueError, match="angle-only"):
        eng.hip.param_shift(args[0], args[3], torch.zeros(K, B, 3, device=cuda))


def test_hea_amp_federated_run_matches_fp32(cuda):
    """Two federated rounds (plain SGD: Adam's normalised steps would amplify last-bit gradient differences of
    near-zero entries) with state_dtype=mfma against fp32: per-round training losses within the train-step bound."""
    from tests.test_fl import small_cfg
    from qfedx_amd.api import run_experiment
    from qfedx_amd.parallel.dist import init_distributed
    dev = torch.device("cuda", 0)
    kw = dict(num_rounds=2, optimizer="sgd", feature_map="amplitude", n_qubits=10, device="cuda", backend="hip")
    outs = {sd: run_experiment(small_cfg(state_dtype=sd, **kw), world=init_distributed(dev), device=dev, backend="hip")
            for sd in ("mfma", "fp32")}
    for a, b in zip(outs["mfma"]["history"], outs["fp32"]["history"]):
        assert np.isfinite(a["train_loss"]) and abs(a["train_loss"] - b["train_loss"]) <= 2e-3, (a, b)
    assert all(np.isfinite(v) for v in outs["mfma"]["accuracies"]) and len(outs["mfma"]["accuracies"]) >= 2


def test_hea_amp_refusals(cuda):
    amp = HeaMfmaProgram(VQCSpec(8, 1, 3, feature_map="amplitude"), cuda, use_spec=False)
    ang = HeaMfmaProgram(VQCSpec(8, 1, 3), cuda, use_spec=False)
    K, B = 1, 2
    th = torch.zeros(K, amp.n_theta, device=cuda)
    x = torch.rand(K, B, 256, device=cuda)
    xa = torch.rand(K, B, 8, device=cuda)
    dm = torch.zeros(K, B, 1, device=cuda)
    w = torch.zeros(K * B, 3, device=cuda)
    with pytest.raises(ValueError, match="complex"):
        amp.expz(dm, th, init=torch.complex(x, x))
    with pytest.raises(ValueError, match="complex"):
        amp.vjp(dm, th, w, init=torch.complex(x, x))
    with pytest.raises(ValueError, match="needs init"):
        amp.expz(dm, th)
    with pytest.raises(ValueError, match="needs init"):
        amp.vjp(dm, th, w)
    with pytest.raises(ValueError, match="angle feature map"):
        ang.expz(xa, th, init=x)
    with pytest.raises(ValueError, match="angle feature map"):
        ang.vjp(xa, th, w, init=x)
    y, wm = torch.zeros(K, B, dtype=torch.long, device=cuda), torch.ones(K, B, device=cuda)
    p = torch.zeros(K, amp.n_theta + 6, device=cuda)
    with pytest.raises(ValueError, match="needs init"):
        amp.loss_and_grads(dm, y, wm, p, amp.spec)
    with pytest.raises(ValueError, match="angle feature map"):
        ang.loss_and_grads(xa, y, wm, p, ang.spec, init=x)
    with pytest.raises(ValueError, match="amplitudes per sample"):
        amp.expz(dm, th, init=torch.rand(K, B, 300, device=cuda))
    with pytest.raises(ValueError, match="eligible_amplitude"):
        HeaMfmaProgram(VQCSpec(8, 1, 3, feature_map="amplitude", entangler="ring"), cuda)
    torch.cuda.synchronize()
