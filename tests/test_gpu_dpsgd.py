"""GPU tests of record-level DP-SGD on the MFMA statevector engine (csrc/hea_dpsgd.hip): the two reductions against
the float64 reference fed with the engine's own per-sample gradients, the whole step against the float64 torch engine,
graphed rounds against eager ones, and the public config path.

Shapes are the smallest at which each mechanism exists (the reason stands next to each case)."""
import math

import pytest
import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops._ext import ext
from qfedx_amd.ops.engine import VQCEngine
from qfedx_amd.ops.hea_mfma import HeaMfmaProgram
from qfedx_amd.privacy.dp import dpsgd_step_ref
from qfedx_amd.utils.seeding import philox_key
from tests.test_fl import small_cfg

pytestmark = pytest.mark.gpu


def _inputs(spec, K, B, seed):
    g = torch.Generator().manual_seed(seed)
    if spec.amplitude:
        init = torch.rand(K, B, 1 << spec.n_qubits, generator=g) + 0.05
        xang = torch.zeros(K, B, spec.x_width)
    else:
        init = None
        xang = spec.encode_features(torch.rand(K, B, spec.n_qubits, generator=g))
    y = torch.randint(0, spec.n_classes, (K, B), generator=g)
    params = torch.stack([spec.init_params(k) for k in range(K)])
    params[:, : spec.n_theta] += 0.5 * torch.randn(K, spec.n_theta, generator=g)
    keys = torch.tensor([philox_key(77, "dpsgd_noise", 1, k) for k in range(K)], dtype=torch.int64)
    return xang, init, y, params, keys


def _slab_rows(hip, params, K, B):
    """Per-sample gradient rows [K, B, P] from the slab and the readout records the last step left in the program's
    workspace, through the route parameter shift already uses: hea_grad_reduce with one sample per 'client'."""
    S, C, nth = K * B, hip.C, hip.n_theta
    gslab = hip._ws["gslab"][: S * hip.slab_tiles * hip.n_gradops * 32]
    rec = hip._ws["rorec"][: S * (2 * C + 2)].view(S, 2 * C + 2)
    th = params.repeat_interleave(B, 0).contiguous()
    g = torch.zeros(S, params.shape[1], dtype=torch.float32, device=params.device)
    ext().hea_grad_reduce(gslab, hip.slab_tiles, hip.n_gradops, hip.gmeta, 1, S, th, g, params.shape[1])
    return torch.cat([g[:, :nth], rec[:, : 2 * C]], -1).view(K, B, nth + 2 * C).double().cpu()


# ------------------------------------------------------------------------------------- (a) kernels vs the engine's own slab
CASES = [
    # n, L, classes, dtype, feature map, entangler, K, B, dead samples / empty clients
    (8, 2, 3, "mfma", "ry", "chain", 2, 3, ()),                 # one pass, partial tile
    (11, 3, 3, "mfma", "ry", "chain", 2, 2, ()),                # pair ops: two regions per op
    (16, 3, 3, "mfma", "ry", "chain", 2, 17, ()),               # 8 slab tiles per op; 136 rows per block: past the
                                                                # unrolled stride (128) and not a multiple of it
    (16, 3, 3, "mfma_bf16", "ry", "chain", 2, 3, ()),           # bf16 storage
    (10, 3, 8, "mfma", "ry", "chain", 3, 4, ()),                # the class maximum
    (12, 3, 3, "mfma", "ry", "chain", 5, 7, ((0, 3), (2, None))),   # one weight-0 sample, one client with an empty lot
    (16, 3, 3, "mfma", "ry", "ring", 1, 2, ()),                 # ring program
    (10, 3, 3, "mfma", "amplitude", "chain", 2, 2, ()),         # amplitude program
]


@pytest.mark.parametrize("n,L,ncls,dtype,feat,ent,K,B,dead", CASES)
def test_dp_kernels_match_reference_on_the_engines_slab(cuda, n, L, ncls, dtype, feat, ent, K, B, dead):
    """grad, norm and c of one DP step against ``dpsgd_step_ref`` fed with the per-sample rows rebuilt from the same
    slab.  The oracle's rows are float32 (2^-24 relative each) and a lot has at most 17 terms, so the gradients agree
    within ~1e-6 x max|grad|: asserted at 1e-5 (a dropped tile or a wrong weight shows at 1e-2 or more); a norm inherits
    2^-24 relative from its rows: asserted at 1e-6 relative, c likewise."""
    spec = VQCSpec(n, L, ncls, feature_map=feat, entangler=ent, readout_scale=2.0)
    eng = VQCEngine(spec, cuda, "hip", dtype)
    assert isinstance(eng.hip, HeaMfmaProgram) and eng.hip.bf16 == (dtype == "mfma_bf16")
    xang, init, y, params, keys = _inputs(spec, K, B, seed=n + K)
    w = torch.full((K, B), 1.0 / B)
    for k, b in dead:
        if b is None:
            w[k] = 0
        else:
            w[k, b] = 0
    live = w > 0
    dev = lambda t: None if t is None else t.to(cuda)
    args = (dev(xang), dev(y), dev(w), dev(params), "adjoint")
    lot = B

    def step(clip, sigma):
        out = eng.loss_and_grads(*args, init=dev(init), dpsgd=dict(clip=clip, sigma=sigma, keys=dev(keys), step=3, lot=lot))
        torch.cuda.synchronize()
        assert "opt_done" not in out
        return {k: v.cpu() for k, v in out.items()}

    step(1.0, 0.0)                                  # the slab does not depend on the clip norm
    rows = _slab_rows(eng.hip, dev(params), K, B)
    assert (rows[~live] == 0).all()                 # a weight-0 sample leaves an all-zero slab row and record
    norms = rows.norm(dim=-1)
    clip = float(norms[live].median())
    plain = eng.loss_and_grads(dev(xang), dev(y), dev(live.float() / live.sum(-1, keepdim=True).clamp(min=1)),
                               dev(params), "adjoint", init=dev(init))
    for sigma in (0.0, 1.0):
        out = step(clip, sigma)
        ref = dpsgd_step_ref(rows, live, clip, sigma, keys, 3, lot)
        assert (ref["c"][live] < 1).any() and (ref["c"][live] == 1).any()          # one clipped, one not
        scale = float(ref["grad"].abs().max())
        err = float((out["grad"].double() - ref["grad"]).abs().max())
        err_n = float(((out["dp_norm"] - ref["norm"]).abs() / ref["norm"].clamp(min=1e-30))[live].max())
        err_c = float((out["dp_c"] - ref["c"]).abs()[live].max())
        print(f"DPSGD_KERNEL n={n} L={L} C={ncls} {dtype} {feat} {ent} K={K} B={B} sigma={sigma} err_g={err:.3e} "
              f"gmax={scale:.3e} err_norm={err_n:.3e} err_c={err_c:.3e}")
        assert err <= 1e-5 * scale, (err, scale)
        assert err_n <= 1e-6 and err_c <= 1e-6, (err_n, err_c)
        assert torch.equal(out["dp_c"][~live], torch.ones(int((~live).sum()), dtype=torch.float64))   # norm 0 -> c = 1
        # loss / hits keep their meaning: the mean CE over the live samples, the hits among them; 0 for an empty lot
        assert torch.allclose(out["loss"], plain["loss"].cpu(), atol=1e-5) and torch.equal(out["correct"], plain["correct"].cpu())
    for k, b in dead:
        if b is None:                               # empty lot: exactly the noise over the lot size
            z = dpsgd_step_ref(rows[k:k + 1] * 0, live[k:k + 1], clip, 1.0, keys[k:k + 1], 3, lot)["grad"][0]
            # (the device's Box-Muller may round an element the other way: one float ulp)
            assert torch.allclose(out["grad"][k], z.float(), rtol=1e-6, atol=0)
            assert out["loss"][k] == 0 and out["correct"][k] == 0


def test_dp_step_refusals(cuda):
    spec = VQCSpec(8, 2, 3)
    xang, _, y, params, keys = (None if t is None else t.to(cuda) for t in _inputs(spec, 1, 2, 0))
    w = torch.ones(1, 2, device=cuda)
    dp = dict(clip=1.0, sigma=1.0, keys=keys, step=0, lot=2)
    with pytest.raises(ValueError, match="VALU"):
        VQCEngine(spec, cuda, "hip").loss_and_grads(xang, y, w, params, "adjoint", dpsgd=dp)
    eng = VQCEngine(spec, cuda, "hip", "mfma")
    with pytest.raises(ValueError, match="grad_method"):
        eng.loss_and_grads(xang, y, w, params, "param_shift", dpsgd=dp)
    with pytest.raises(ValueError, match="keys"):
        eng.loss_and_grads(xang, y, w, params, "adjoint", dpsgd=dict(dp, keys=None))
    with pytest.raises(ValueError, match="noiseless"):           # any readout noise model: no per-sample record
        eng.hip.loss_and_grads(xang, y, w, params, spec, object(), keys, dpsgd=dp)


# ------------------------------------------------------------------------------------- (b) end to end vs float64
def e2e_errors(cuda, n, L, dtype, K=2, B=4):
    """(max |grad - grad64|, max |norm - norm64| / norm64) of one DP step (sigma = 1, C = the float64 median norm)
    against the torch engine in float64 on the same inputs."""
    spec = VQCSpec(n, L, 3, readout_scale=2.0)
    xang, _, y, params, keys = _inputs(spec, K, B, seed=100 + n)
    w = torch.ones(K, B)
    ref_eng = VQCEngine(spec, "cpu", "torch")
    p64 = params.double()
    dp = dict(clip=1.0, sigma=1.0, keys=keys, step=1, lot=B)
    clip = float(ref_eng.loss_and_grads(xang.double(), y, w, p64, "autograd", dpsgd=dp)["dp_norm"].median())
    dp["clip"] = clip
    ref = ref_eng.loss_and_grads(xang.double(), y, w, p64, "autograd", dpsgd=dp)
    out = VQCEngine(spec, cuda, "hip", dtype).loss_and_grads(xang.to(cuda), y.to(cuda), w.to(cuda), params.to(cuda),
                                                             "adjoint", dpsgd=dict(dp, keys=keys.to(cuda)))
    torch.cuda.synchronize()
    eg = float((out["grad"].double().cpu() - ref["grad"].double()).abs().max())
    en = float(((out["dp_norm"].cpu() - ref["dp_norm"]).abs() / ref["dp_norm"]).max())
    return eg, en


# measured on an MI355X (profiles/dpsgd_err_table.txt): (max |d grad|, max |d norm| / norm); asserted at 3 x
E2E_MEASURED = {(8, 2, "mfma"): (7.617e-05, 1.993e-04), (8, 2, "mfma_bf16"): (1.100e-03, 2.810e-03),
                (12, 3, "mfma"): (5.781e-05, 1.439e-04), (12, 3, "mfma_bf16"): (5.515e-04, 1.111e-03),
                (16, 3, "mfma"): (3.197e-05, 8.314e-05), (16, 3, "mfma_bf16"): (2.483e-04, 3.761e-04)}


@pytest.mark.parametrize("n,L", [(8, 2), (12, 3), (16, 3)])
@pytest.mark.parametrize("dtype", ["mfma", "mfma_bf16"])
def test_dp_step_matches_float64_engine(cuda, n, L, dtype):
    eg, en = e2e_errors(cuda, n, L, dtype)
    mg, mn = E2E_MEASURED[(n, L, dtype)]
    print(f"DPSGD_E2E n={n} L={L} {dtype} err_grad={eg:.3e} (bound {3 * mg:.3e}) err_norm_rel={en:.3e} (bound {3 * mn:.3e})")
    assert eg <= 3 * mg, (eg, mg)
    assert en <= 3 * mn, (en, mn)


# ------------------------------------------------------------------------------------- (c) graph replay, (d) public path
def _cfg(**kw):
    base = {"model.n_qubits": 10, "model.n_layers": 3, "num_clients": 4, "samples_per_client": 32, "batch_size": 8,
            "local_steps": 2, "test_samples": 32, "runtime.device": "cuda", "runtime.backend": "hip", "dp": True,
            "privacy.level": "record", "deterministic_noise": True, "noise_multiplier": 1.0, "num_rounds": 2}
    return small_cfg(**{**base, **kw})


def _two_rounds(cfg, freeze_keys=False):
    from tests.test_dpsgd import _runner
    runner = _runner(cfg)
    if freeze_keys:                      # the mistake the device key table exists to prevent: round 0's keys forever
        tables = runner._dpsgd_tables
        runner._dpsgd_tables = lambda r, ids: tables(0, ids)
    out = []
    for r in range(2):
        rec = runner.run_round(r)
        torch.cuda.synchronize()
        out.append(runner.params.clone().cpu())
        assert rec["dp_level"] == "record" and math.isfinite(rec["train_loss"])
    return out, runner


def test_graphed_dp_rounds_equal_eager_rounds_bitwise(cuda):
    eager, _ = _two_rounds(_cfg(**{"runtime.use_graphs": False}))
    graphed, runner = _two_rounds(_cfg(**{"runtime.use_graphs": True}))
    assert len(runner.adapter.trainer._graph_cache) == 1            # round 1 replayed round 0's capture
    assert torch.equal(graphed[0], eager[0]) and torch.equal(graphed[1], eager[1])
    # the check is sensitive to a frozen key: rounds that reuse round 0's keys end elsewhere
    k0, k1 = runner._dpsgd_tables(0, [0, 1, 2, 3])["dpsgd_keys"], runner._dpsgd_tables(1, [0, 1, 2, 3])["dpsgd_keys"]
    assert not torch.equal(k0, k1)
    frozen, _ = _two_rounds(_cfg(**{"runtime.use_graphs": False}), freeze_keys=True)
    assert torch.equal(frozen[0], eager[0]) and not torch.equal(frozen[1], eager[1])


def test_run_experiment_record_level_on_hip(cuda):
    from qfedx_amd.api import run_experiment
    out = run_experiment(_cfg())
    assert out["backend"] == "hip"
    rec = out["history"][-1]
    assert math.isfinite(rec["train_loss"]) and rec["dp_level"] == "record" and rec["epsilon"] > 0
    assert rec["dp_lot_overflow"] == 0 and torch.isfinite(out["params"]).all()
