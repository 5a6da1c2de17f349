"""Cases, inputs and float64 references of the GPU quantum-natural-gradient tests (tests/test_gpu_qng.py,
tools/qng_err_table.py).  Everything here runs on the CPU; references are computed once and shared.

``MEASURED`` holds the errors of the kernels against these references on one MI355X, as profiles/qng_err_table.txt
records them; a test's bound is 3 x its case's figure (the project's convention)."""
import functools
import math

import torch

from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import qng

# ---- 1. correlator kernel: qubit counts on both sides of every boundary of csrc/qng.hip qng_corr_tile_kernel --------
# index bit 0 sits in a lane's registers, bits 1..6 in the lane id, bits 7..8 in the wave id, bits 9..10 in the lane's
# four 16-byte loads, bits >= 11 in the tile id: n = 7 | 8 crosses the wave, 9 | 10 the load count, 11 | 12 the tile (12:
# exactly one high bit -> low x high pairs, 13: two -> high x high pairs), 16: 32 tiles
CORR_N = (2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 16)


def corr_samples(n: int) -> int:
    return 2 if n == 16 else 3


@functools.lru_cache(maxsize=None)
def corr_states(n: int) -> torch.Tensor:
    """Random normalised complex64 states [S, 2^n]."""
    g = torch.Generator().manual_seed(100 + n)
    st = torch.randn(corr_samples(n), 1 << n, 2, generator=g, dtype=torch.float64)
    st = torch.view_as_complex(st)
    return (st / st.abs().pow(2).sum(-1, keepdim=True).sqrt()).to(torch.complex64)


@functools.lru_cache(maxsize=None)
def corr_reference(n: int):
    """(<Z_i> [S, n], <Z_i Z_j> [S, n, n]) in float64 from the complex64 amplitudes the kernel reads."""
    return qng.z_correlators(corr_states(n), n)


def unpack_record(rec: torch.Tensor, n: int):
    """rec [.., n (n + 1) / 2] -> (z [.., n], zz pairs [.., n (n - 1) / 2], index vectors i, j)."""
    i, j = qng.pair_rows(n)
    return rec[..., :n], rec[..., n:], i, j


# ---- 2. metric_blocks: (name, qubits, layers, entangler, feature map) ------------------------------------------------
METRIC_CASES = (("4q2L_chain_ry", 4, 2, "chain", "ry"), ("8q2L_ring_rx", 8, 2, "ring", "rx"),
                ("10q1L_none_rz", 10, 1, "none", "rz"), ("8q2L_chain_amp", 8, 2, "chain", "amplitude"),
                ("13q3L_chain_ry", 13, 3, "chain", "ry"))
METRIC_K, METRIC_B = 2, 3


def metric_spec(name: str) -> VQCSpec:
    _, n, L, ent, fm = next(c for c in METRIC_CASES if c[0] == name)
    return VQCSpec(n_qubits=n, n_layers=L, n_classes=3, feature_map=fm, entangler=ent)


@functools.lru_cache(maxsize=None)
def metric_inputs(name: str) -> dict:
    """float32 inputs: xang [K, B, x_width], params [K, P], init (amplitude) or None, wmask [K, B] with one dead sample
    in client 0 and client 1 all dead."""
    spec = metric_spec(name)
    K, B = METRIC_K, METRIC_B
    g = torch.Generator().manual_seed(sum(name.encode()))
    params = torch.cat([torch.randn(K, spec.n_theta, generator=g) * 0.8, torch.ones(K, spec.n_classes),
                        torch.zeros(K, spec.n_classes)], -1)
    if spec.amplitude:
        init = torch.randn(K, B, 1 << spec.n_qubits, generator=g)
        xang = torch.zeros(K, B, 1)
    else:
        init = None
        xang = torch.rand(K, B, spec.n_qubits, generator=g) * math.pi
    wmask = torch.tensor([[0.5, 0.0, 0.5], [0.0, 0.0, 0.0]])
    return {"xang": xang, "params": params, "init": init, "wmask": wmask}


@functools.lru_cache(maxsize=None)
def metric_reference(name: str) -> dict:
    """per-sample blocks [K, B, 2L, n, n] and client blocks [K, 2L, n, n] of the float64 oracle."""
    spec, inp = metric_spec(name), metric_inputs(name)
    per = qng.fubini_study_blocks(spec, inp["xang"], inp["params"][:, :spec.n_theta], inp["init"])
    return {"per_sample": per, "blocks": qng.client_blocks(per, inp["wmask"])}


# ---- 3. step kernel --------------------------------------------------------------------------------------------------
STEP_N = (2, 7, 16, 32)
STEP_K, STEP_B, STEP_L = 3, 4, 2
STEP_LR, STEP_DAMPING = 0.05, 1e-3


@functools.lru_cache(maxsize=None)
def step_inputs(n: int) -> dict:
    """Records of classical bit-string mixtures (their covariance blocks are positive semi-definite): rec [K * B, 2L,
    n (n + 1) / 2] float64, wmask [K, B] (one dead sample per client), params / grad [K, P] float32, active [K] (row 2
    inactive).  Block 2 of client 1 is exactly zero: its live samples are single bit strings."""
    spec = VQCSpec(n_qubits=n, n_layers=STEP_L, n_classes=2)
    K, B, nb, M = STEP_K, STEP_B, 2 * STEP_L, 5
    g = torch.Generator().manual_seed(300 + n)
    s = (torch.randint(0, 2, (K, B, nb, M, n), generator=g) * 2 - 1).double()
    p = torch.rand(K, B, nb, M, generator=g, dtype=torch.float64)
    p[1, :, 2, 1:] = 0.0
    p = p / p.sum(-1, keepdim=True)
    z = (p.unsqueeze(-1) * s).sum(-2)                                       # [K, B, nb, n]
    zz = torch.einsum("kbcm,kbcmi,kbcmj->kbcij", p, s, s)
    i, j = qng.pair_rows(n)
    rec = torch.cat([z, zz[..., i, j]], -1).reshape(K * B, nb, -1).contiguous()
    wmask = torch.full((K, B), 1.0 / (B - 1))
    wmask[:, 1] = 0.0
    params = torch.randn(K, spec.n_params, generator=g)
    grad = torch.randn(K, spec.n_params, generator=g) * 0.3
    return {"spec": spec, "rec": rec, "wmask": wmask, "params": params, "grad": grad,
            "active": torch.tensor([1.0, 1.0, 0.0])}


@functools.lru_cache(maxsize=None)
def step_reference(n: int) -> dict:
    inp = step_inputs(n)
    spec = inp["spec"]
    per = qng.records_to_blocks(inp["rec"], n).reshape(STEP_K, STEP_B, 2 * STEP_L, n, n)
    G = qng.client_blocks(per, inp["wmask"])
    out = inp["params"].clone()
    qng.qng_step_ref(out, inp["grad"], G, inp["active"], STEP_LR, STEP_DAMPING, spec)
    return {"blocks": G, "params": out}


# ---- measured on one MI355X (profiles/qng_err_table.txt): max |kernel - float64 reference| per case -------------------
MEASURED = {
    "corr_2_z": 6.339e-08,
    "corr_2_zz": 5.231e-08,
    "corr_3_z": 5.763e-08,
    "corr_3_zz": 2.820e-08,
    "corr_6_z": 6.443e-08,
    "corr_6_zz": 3.425e-08,
    "corr_7_z": 2.015e-08,
    "corr_7_zz": 3.070e-08,
    "corr_8_z": 4.152e-08,
    "corr_8_zz": 3.579e-08,
    "corr_9_z": 5.093e-08,
    "corr_9_zz": 2.116e-08,
    "corr_10_z": 5.003e-08,
    "corr_10_zz": 3.125e-08,
    "corr_11_z": 3.586e-08,
    "corr_11_zz": 2.279e-08,
    "corr_12_z": 4.908e-08,
    "corr_12_zz": 2.428e-08,
    "corr_13_z": 2.968e-08,
    "corr_13_zz": 4.820e-08,
    "corr_16_z": 2.172e-08,
    "corr_16_zz": 1.440e-08,
    "metric_4q2L_chain_ry_blocks": 1.004e-07,
    "metric_4q2L_chain_ry_per_sample": 2.894e-07,
    "metric_8q2L_ring_rx_blocks": 1.114e-07,
    "metric_8q2L_ring_rx_per_sample": 2.181e-07,
    "metric_10q1L_none_rz_blocks": 1.633e-07,
    "metric_10q1L_none_rz_per_sample": 3.570e-07,
    "metric_8q2L_chain_amp_blocks": 1.289e-08,
    "metric_8q2L_chain_amp_per_sample": 3.492e-08,
    "metric_13q3L_chain_ry_blocks": 3.829e-07,
    "metric_13q3L_chain_ry_per_sample": 5.305e-07,
    "step_2_params": 0.000e+00,
    "step_2_blocks": 5.551e-17,
    "step_7_params": 0.000e+00,
    "step_7_blocks": 5.551e-17,
    "step_16_params": 1.907e-06,
    "step_16_blocks": 5.551e-17,
    "step_32_params": 0.000e+00,
    "step_32_blocks": 5.551e-17,
    "round_fp32_params": 6.258e-07,
    "round_mfma_params": 8.523e-06,
}


def bound(key: str) -> float:
    """3 x the case's measured error."""
    return 3.0 * MEASURED[key]
