"""Quantum natural gradient on the GPU: the correlator and step kernels (csrc/qng.hip), the engine's metric pass and a
federated round against the float64 oracle of ops/qng.py.

Bounds are 3 x the error measured per case on one MI355X (tests/qng_cases.py MEASURED, recorded by
tools/qng_err_table.py in profiles/qng_err_table.txt); every test prints its figures before it asserts."""
import functools

import pytest
import torch

from qfedx_amd.fl.optim import BatchedOptimizer
from qfedx_amd.ops import qng
from qfedx_amd.ops.engine import VQCEngine
from tests import qng_cases as qc
from tests.test_fl import small_cfg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ 1. correlator kernel
def corr_records(n: int, states: torch.Tensor = None) -> torch.Tensor:
    """rec [S, n (n + 1) / 2] float64 of ``qng_corr`` on the case's states (cpu)."""
    from qfedx_amd.ops._ext import ext
    C = ext()
    st = (qc.corr_states(n) if states is None else states).to(DEV).contiguous()
    S = st.shape[0]
    trec = torch.full((S * int(C.qng_tiles(n)) * int(C.qng_tile_rec()),), float("nan"), device=DEV)
    rec = torch.full((S + 1, 2, n * (n + 1) // 2), float("nan"), dtype=torch.float64, device=DEV)
    C.qng_corr(st, n, trec, rec, 0, 1)
    torch.cuda.synchronize()
    assert rec[:, 0].isnan().all() and rec[S].isnan().all(), "qng_corr wrote outside its rows / cut"
    return rec[:S, 1].cpu()


def corr_errors(n: int) -> dict:
    z_ref, zz_ref = qc.corr_reference(n)
    z, zz, i, j = qc.unpack_record(corr_records(n), n)
    return {"z": (z - z_ref).abs().max().item(), "zz": (zz - zz_ref[:, i, j]).abs().max().item()}


@pytest.mark.parametrize("n", qc.CORR_N)
def test_correlator_kernel_matches_float64(cuda, n):
    err = corr_errors(n)
    print(f"qng_corr n={n}: {err}")
    _, zz_ref = qc.corr_reference(n)
    assert zz_ref.abs().max().item() > 1e-3, "degenerate case"
    assert err["z"] <= qc.bound(f"corr_{n}_z") and err["zz"] <= qc.bound(f"corr_{n}_zz")


def test_correlator_record_does_not_depend_on_launch_mates(cuda):
    """A sample's record is the same bits alone, among others and on a repeat (n = 12: two tiles)."""
    n = 12
    st = qc.corr_states(n)
    full = corr_records(n)
    assert torch.equal(full, corr_records(n))
    for s in range(st.shape[0]):
        assert torch.equal(corr_records(n, st[s:s + 1])[0], full[s])


# ------------------------------------------------------------------------------------------------ 2. metric_blocks
@functools.lru_cache(maxsize=None)
def metric_run(name: str) -> dict:
    spec, inp = qc.metric_spec(name), qc.metric_inputs(name)
    eng = VQCEngine(spec, DEV, "hip")
    args = [inp["xang"].to(DEV), inp["wmask"].to(DEV), inp["params"].to(DEV),
            None if inp["init"] is None else inp["init"].to(DEV)]
    G = eng.metric_blocks(*args)
    rec = eng.metric_records(*args)["rec"]
    torch.cuda.synchronize()
    return {"engine": eng, "args": args, "blocks": G.cpu(), "rec": rec.cpu()}


def metric_errors(name: str) -> dict:
    spec, ref, run = qc.metric_spec(name), qc.metric_reference(name), metric_run(name)
    per = qng.records_to_blocks(run["rec"], spec.n_qubits).reshape(ref["per_sample"].shape)
    return {"blocks": (run["blocks"] - ref["blocks"]).abs().max().item(),
            "per_sample": (per - ref["per_sample"]).abs().max().item()}


@pytest.mark.parametrize("name", [c[0] for c in qc.METRIC_CASES])
def test_metric_blocks_match_the_oracle(cuda, name):
    err = metric_errors(name)
    print(f"metric_blocks {name}: {err}")
    G, ref = metric_run(name)["blocks"], qc.metric_reference(name)["blocks"]
    assert G.dtype == torch.float64 and G.shape == ref.shape
    assert torch.equal(G[1], torch.zeros_like(G[1])), "a client without a live sample gets zero blocks"
    assert ref[0].abs().max().item() > 1e-2, "degenerate case"
    assert err["blocks"] <= qc.bound(f"metric_{name}_blocks")
    assert err["per_sample"] <= qc.bound(f"metric_{name}_per_sample")


# ------------------------------------------------------------------------------------------------ 3. step kernel
def step_run(n: int, rows=slice(None)) -> torch.Tensor:
    """params after the HIP step on client rows ``rows`` of the case (cpu)."""
    inp = qc.step_inputs(n)
    B, nb = qc.STEP_B, 2 * qc.STEP_L
    rec = inp["rec"].reshape(qc.STEP_K, B, nb, -1)[rows].reshape(-1, nb, inp["rec"].shape[-1]).contiguous()
    params = inp["params"][rows].clone().to(DEV)
    opt = BatchedOptimizer("qng", params.shape, DEV, qc.STEP_LR, backend="hip", damping=qc.STEP_DAMPING,
                           spec=inp["spec"])
    opt.step(params, inp["grad"][rows].to(DEV), inp["active"][rows].to(DEV),
             metric={"rec": rec.to(DEV), "wmask": inp["wmask"][rows].contiguous().to(DEV)})
    torch.cuda.synchronize()
    return params.cpu()


def step_errors(n: int) -> dict:
    from qfedx_amd.ops._ext import ext
    inp, ref = qc.step_inputs(n), qc.step_reference(n)
    G = torch.empty(qc.STEP_K, 2 * qc.STEP_L, n, n, dtype=torch.float64, device=DEV)
    ext().qng_blocks(inp["rec"].to(DEV), inp["wmask"].to(DEV), n, G)
    return {"params": (step_run(n).double() - ref["params"].double()).abs().max().item(),
            "blocks": (G.cpu() - ref["blocks"]).abs().max().item()}


@pytest.mark.parametrize("n", qc.STEP_N)
def test_step_kernel_matches_the_reference(cuda, n):
    err = step_errors(n)
    print(f"qng_step n={n}: {err}")
    inp, ref = qc.step_inputs(n), qc.step_reference(n)
    assert torch.equal(ref["blocks"][1, 2], torch.zeros(n, n, dtype=torch.float64)), "the case lost its zero block"
    out = step_run(n)
    assert torch.equal(out[2], inp["params"][2]), "the inactive row changed"
    assert not torch.equal(out[0], inp["params"][0])
    assert err["params"] <= qc.bound(f"step_{n}_params") and err["blocks"] <= qc.bound(f"step_{n}_blocks")


# ------------------------------------------------------------------------------------------------ 4. bitwise
def test_step_is_bitwise_repeatable_and_independent_of_batch_mates(cuda):
    for n in (7, 32):
        full = step_run(n)
        assert torch.equal(full, step_run(n))
        assert torch.equal(step_run(n, slice(1, 2))[0], full[1])


@pytest.mark.parametrize("name", ["8q2L_ring_rx", "8q2L_chain_amp", "13q3L_chain_ry"])
def test_metric_records_are_bitwise_under_repeats_mates_and_chunking(cuda, name):
    run = metric_run(name)
    eng, (xang, wmask, params, init) = run["engine"], run["args"]
    assert torch.equal(eng.metric_records(xang, wmask, params, init)["rec"].cpu(), run["rec"])
    B = qc.METRIC_B
    alone = eng.metric_records(xang[:1], wmask[:1], params[:1], None if init is None else init[:1])["rec"].cpu()
    assert torch.equal(alone, run["rec"][:B])
    small = VQCEngine(qc.metric_spec(name), DEV, "hip")
    small._budget = 2 * 16 * (1 << small.spec.n_qubits)                # two samples per chunk: three chunks
    assert torch.equal(small.metric_records(xang, wmask, params, init)["rec"].cpu(), run["rec"])
    assert small._metric_prog._ws["psi"].numel() == 2 << small.spec.n_qubits
    small._budget = 16 * (1 << small.spec.n_qubits) - 1
    with pytest.raises(ValueError, match="model.n_qubits"):
        small.metric_records(xang, wmask, params, init)


# ------------------------------------------------------------------------------------------------ 5. a federated round
ROUND_KW = {"num_rounds": 1, "model.n_qubits": 8, "model.n_layers": 2, "train.optimizer": "qng",
            "train.learning_rate": 0.05}


@functools.lru_cache(maxsize=None)
def round_params(backend: str, state_dtype: str = "fp32", graphs: bool = True) -> torch.Tensor:
    from qfedx_amd.api import run_experiment
    kw = dict(ROUND_KW, **{"runtime.backend": backend, "model.state_dtype": state_dtype,
                           "runtime.device": "cuda" if backend == "hip" else "cpu", "runtime.use_graphs": graphs})
    return run_experiment(small_cfg(**kw))["params"].detach().cpu()


def round_errors(state_dtype: str) -> dict:
    return {"params": (round_params("hip", state_dtype).double() - round_params("torch").double()).abs().max().item()}


@pytest.mark.parametrize("state_dtype", ["fp32", "mfma"])
def test_local_round_matches_the_torch_backend(cuda, state_dtype):
    err = round_errors(state_dtype)
    print(f"qng round 8q x 2L, state_dtype={state_dtype}: {err}")
    start = small_cfg(**ROUND_KW)
    from qfedx_amd.models.vqc import VQCSpec
    p0 = VQCSpec(8, 2, start.model.n_classes, readout_scale=start.model.readout_scale).init_params(start.train.seed)
    assert (round_params("torch") - p0).abs().max().item() > 1e-3, "the round did not move the model"
    assert err["params"] <= qc.bound(f"round_{state_dtype}_params")


@pytest.mark.parametrize("state_dtype", ["fp32", "mfma"])
def test_use_graphs_true_and_false_are_bitwise(cuda, state_dtype):
    assert torch.equal(round_params("hip", state_dtype, True), round_params("hip", state_dtype, False))


# ------------------------------------------------------------------------------------------------ 6. run_experiment
def test_run_experiment_hip_qng(cuda):
    import math
    import os
    from qfedx_amd.api import run_experiment
    from qfedx_amd.config import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", "iris_4q_qng.yaml"),
                      ["train.num_rounds=2", "runtime.backend=hip", "runtime.device=cuda", "runtime.log_every=100"])
    out = run_experiment(cfg)
    hist = [h for h in out["history"] if "train_loss" in h]
    assert len(hist) == 2 and all(math.isfinite(h["train_loss"]) for h in hist)
    assert torch.isfinite(out["params"]).all()
