"""CPU tests of the MFMA engine's amplitude mode: the planner runs layer 1 as a rotation layer over a stored input
state (``build_plan(feature="amplitude")``), the emulator starts from ``init``, the numpy reference of the staging
kernel, and the routing that keeps ``auto`` / ``bf16`` amplitude specs on the VALU engine."""
import numpy as np
import pytest
import torch

from qfedx_amd.fl.adapters import resolve_state_dtype
from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_plan as hp
from qfedx_amd.ops.statevec_torch import TorchProgram, slot_grads

SHAPES = [(8, 1, 14), (10, 2, 14), (12, 2, 10), (15, 2, 14), (16, 3, 14)]


def _plan(n, L, t, readout=None, chain=True):
    return hp.build_plan(n, L, list(range(3)) if readout is None else readout, chain, "amplitude", tile_bits=t)


def _dense(spec, states, params, wread):
    """float64 dense simulation started from ``states`` [K, B, 2^n] complex128."""
    ops, coef = spec.program()
    prog = TorchProgram(ops, coef, spec.n_qubits, dtype=torch.complex128)
    K, B, _ = states.shape
    P = spec.n_theta
    xz = torch.zeros(K, B, spec.x_width, dtype=torch.float64)
    rows = torch.cat([params[:, None, :P].expand(K, B, P), xz], -1).reshape(K * B, -1)
    psi = prog.run(rows, state=states.reshape(K * B, -1))
    ez = prog.expz(psi, spec.readout).reshape(K, B, -1)
    g = prog.adjoint_grads(rows, psi, wread.reshape(K * B, -1), spec.readout)
    return ez.numpy(), slot_grads(g, prog.ops, prog.coef, rows.shape[1])[:, :P].reshape(K, B, P).sum(1).numpy()


@pytest.mark.parametrize("n,L,t", SHAPES)
def test_amplitude_plan_structure(n, L, t):
    plan = _plan(n, L, t)
    assert plan.amplitude and plan.first_layer == 1
    assert all(not p.l1 for p in plan.passes)
    seen = []
    order = {}                                   # (layer, qubit) -> position in the execution order
    pos = 0
    for p in plan.passes:
        for g in p.groups:
            assert 1 <= g.layer <= L and g.frame == plan.layer_frame(g.layer)
            assert (g.support(n) & ~p.mask()) == 0, "group support leaves its pass tile"
            for q in g.qubits:
                seen += [plan.theta_slot(g.layer, q), plan.theta_slot(g.layer, q) + 1]
                order[(g.layer, q)] = pos
            pos += 1
    assert sorted(seen) == list(range(plan.n_theta)), "every theta index in exactly one rotation group"
    for (layer, q), at in order.items():
        if layer == 1:
            assert hp.frame_vec(q, 0, n) == 1 << q
            continue
        s = hp.frame_vec(q, plan.layer_frame(layer), n)
        for r in range(n):
            if hp.frame_vec(r, plan.layer_frame(layer - 1), n) & s:
                assert order[(layer - 1, r)] < at, "a rotation ran before an overlapping one of the layer below"
    meta = []
    for _, fwd, adj in hp.pass_programs(plan, meta):
        codes = [int(w[hp.W_CODE]) for w in adj]
        assert hp.OP_GRAD_L1 not in codes and hp.OP_GRAD2 not in codes
        assert all(int(w[hp.W_CODE]) in (hp.OP_APPLY, hp.OP_APPLY2, hp.OP_READOUT) for w in fwd)
    owned = []
    for row in meta:
        nr = int(row[1]) & 15
        owned += [int(v) for v in row[2:2 + nr]] + [int(v) for v in row[6:6 + nr]]
    assert sorted(owned) == list(range(plan.n_theta))


def test_issue_plan_shapes():
    """Pass and group counts the planner mode was designed against."""
    count = lambda pl: (len(pl.passes), sum(len(p.groups) for p in pl.passes))
    assert count(_plan(8, 1, 14)) == (1, 2)
    assert count(_plan(10, 3, 14)) == (1, 9)
    p12 = _plan(12, 2, 10)
    assert len(p12.passes) == 2
    last = p12.passes[1]
    assert last.hi == 12 and last.lo <= 10 and last.t == 10     # a strided tile over the top bits
    assert any(g.layer == 1 and set(g.qubits) >= {10, 11} for g in last.groups)
    assert len(_plan(15, 2, 14).passes) == 2
    p16 = count(_plan(16, 3, 14))                # (greedy: 15 groups; trimming layer tails may save some)
    assert p16[0] == 2 and 12 <= p16[1] <= 15
    assert len(_plan(20, 2, 14).passes) == 2


@pytest.mark.parametrize("pair", ["7", "0"])
@pytest.mark.parametrize("n,L,t,B,readout", [(8, 1, 14, 2, None), (10, 2, 14, 2, [0, 4, 9]), (12, 2, 10, 2, None),
                                             (15, 2, 14, 1, None)])
def test_emulated_amplitude_plan_matches_dense(n, L, t, B, readout, pair, monkeypatch):
    monkeypatch.setenv("QFEDX_HEA_PAIR", pair)
    K = 2 if n < 15 else 1
    spec = VQCSpec(n, L, 3, feature_map="amplitude", readout=readout)
    plan = hp.build_plan(n, L, spec.readout, True, "amplitude", tile_bits=t)
    codes = {int(w[hp.W_CODE]) for _, f, a in hp.pass_programs(plan) for w in list(f) + list(a)}
    assert not codes & set(hp.PAIR_CODES) if pair == "0" or plan.t < 11 else hp.OP_APPLY2 in codes
    g = torch.Generator().manual_seed(n * 10 + L)
    x = torch.randn(K, B, 1 << n, generator=g, dtype=torch.float64)
    x[0, 0, (1 << n) // 3:] = 0.0                # a padded (short) row
    states = spec.initial_states(x).to(torch.complex128)
    params = torch.randn(K, spec.n_params, generator=g, dtype=torch.float64)
    wr = torch.randn(K, B, 3, generator=g, dtype=torch.float64)
    ez, gr = _dense(spec, states, params, wr)
    ez2, gr2 = hp.emulate(plan, None, params.numpy(), wr.numpy(), init=states.numpy())
    np.testing.assert_allclose(ez2, ez, atol=1e-12)
    np.testing.assert_allclose(gr2, gr, atol=1e-12)
    if n <= 12:
        ez3, gr3 = hp.emulate(plan, None, params.numpy(), wr.numpy(), fp16=True, init=states.numpy())
        np.testing.assert_allclose(ez3, ez, atol=2e-3)
        np.testing.assert_allclose(gr3, gr, atol=3e-3 * max(1.0, np.abs(gr).max()))


def test_emulate_refuses_a_mismatched_start():
    amp, ang = _plan(8, 1, 14), hp.build_plan(8, 1, [0, 1, 2], True, "ry")
    th = np.zeros((1, amp.n_theta + 6))
    with pytest.raises(ValueError):
        hp.emulate(amp, np.zeros((1, 1, 8)), th)
    with pytest.raises(ValueError):
        hp.emulate(ang, np.zeros((1, 1, 8)), th, init=np.ones((1, 1, 256)) / 16)


def test_eligibility_predicates():
    amp = lambda n=8, C=3, **kw: VQCSpec(n, 2, C, feature_map="amplitude", **kw)
    assert not hp.eligible(amp())                               # unchanged: auto keeps these on the VALU engine
    assert not hp.eligible(amp(entangler="none"))
    assert hp.eligible_amplitude(amp()) and hp.eligible_amplitude(amp(entangler="none"))
    assert not hp.eligible_amplitude(amp(entangler="ring"))
    assert not hp.eligible_amplitude(amp(noisy=True))
    assert not hp.eligible_amplitude(amp(n=7))
    assert not hp.eligible_amplitude(amp(n=9, C=9))
    assert not hp.eligible_amplitude(VQCSpec(8, 2, 3))          # an angle spec is the other predicate's


def test_auto_and_bf16_routing_unchanged():
    spec = VQCSpec(10, 2, 3, feature_map="amplitude")
    assert resolve_state_dtype("auto", spec, "hip", None) == "fp32"
    assert resolve_state_dtype("bf16", spec, "hip", None) == "bf16"
    for explicit in ("mfma", "fp16", "mfma_bf16"):
        assert resolve_state_dtype(explicit, spec, "hip", None) == explicit


def _sig(plan):
    return (plan.feature, plan.t, plan.n_slots,
            [(p.c, p.lo, p.hi, list(p.H), sorted(p.cols.items()),
              [(g.layer, tuple(g.qubits), g.frame, g.slot) for g in p.groups],
              [(g.layer, tuple(g.qubits), g.frame, g.slot) for g in p.l1]) for p in plan.passes])


@pytest.mark.parametrize("n,L", [(10, 2), (12, 3)])
def test_angle_plan_unaffected_by_amplitude_plan(n, L):
    hp._PLAN_CACHE.clear()
    before = hp.build_plan(n, L, [0, 1, 2], True, "ry")
    hp._PLAN_CACHE.clear()
    amp = _plan(n, L, hp.TILE_BITS)
    after = hp.build_plan(n, L, [0, 1, 2], True, "ry")
    assert not after.amplitude and after.first_layer == 2
    assert _sig(after) == _sig(before) and _sig(after) != _sig(amp)
    assert any(p.l1 for p in after.passes)
    for (_, f0, a0), (_, f1, a1) in zip(hp.pass_programs(before), hp.pass_programs(after)):
        assert np.array_equal(f0, f1) and np.array_equal(a0, a1)


@pytest.mark.parametrize("storage", ["fp16", "bf16"])
def test_amp_stage_reference(storage):
    n, F = 8, 200
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, F)).astype(np.float32)
    x[1] = 0.0
    x[2] = 0.0
    x[2, 7] = -3.0                                # one-hot: +- 2^(n // 2) exactly
    x[3] = np.where(rng.random(F) < 0.8, 0.0, rng.random(F)).astype(np.float32)
    ref = hp.amp_stage_ref(x, n, storage)
    assert ref.shape == (4, 256) and np.all(ref[:, F:][[0, 2, 3]] == 0.0)
    assert np.all(ref[1] == 1.0)                  # uniform: 2^(n/2) / sqrt(2^n)
    assert ref[2, 7] == -16.0 and np.count_nonzero(ref[2]) == 1
    exact = x[0].astype(np.float64) / np.sqrt((x[0].astype(np.float64) ** 2).sum()) * 16.0
    ulp = 2.0 ** (-10 if storage == "fp16" else -7)
    assert np.all(np.abs(ref[0, :F] - exact) <= ulp * np.maximum(np.abs(exact), 2.0 ** -14))
    # the staged state is what the emulator starts from: normalised init, scaled and rounded once
    rnd = hp._round16 if storage == "fp16" else hp._round_bf16
    st = VQCSpec(n, 1, 3, feature_map="amplitude").initial_states(torch.from_numpy(x)).numpy().astype(np.complex128)
    assert np.abs(rnd(st * 16.0).real - ref).max() <= ulp * 16.0
    with pytest.raises(ValueError):
        hp.amp_stage_ref(np.zeros((1, 257), np.float32), n)
