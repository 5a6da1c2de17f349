"""CPU tests of the MFMA engine's ring mode: the GF(2) frames of a ring entangler, the exact commutation DAG and the
layer-1 gradient rule of the ring planner (``build_plan(ring=True)``), its plans emulated tile by tile against the dense
float64 oracle, the routing predicates, and digests showing that chain / no-entangler plans are what they were."""
import functools
import hashlib

import numpy as np
import pytest
import torch

from qfedx_amd.fl.adapters import resolve_state_dtype
from qfedx_amd.models.vqc import VQCSpec
from qfedx_amd.ops import hea_plan as hp
from qfedx_amd.ops.statevec_torch import TorchProgram, slot_grads

# (n, L, tile bits, feature): the shapes the ring mode was prototyped on
PROTO = [(8, 2, 8, "ry"), (10, 3, 8, "ry"), (9, 3, 8, "rx"), (10, 2, 8, "amplitude"), (11, 3, 9, "ry"),
         (12, 3, 11, "ry"), (12, 3, 10, "amplitude"), (13, 2, 12, "amplitude")]
BIG = [(n, L, 14, f) for (n, L) in ((16, 3), (20, 2), (16, 2)) for f in ("ry", "amplitude")]


def _readout(n):
    return [0, n // 2, n - 1]


def _plan(n, L, t, feat):
    return hp.build_plan(n, L, _readout(n), feature=feat, tile_bits=t, ring=True)


def _par(x):
    return bin(x).count("1") & 1


# ------------------------------------------------------------------------------------------------ frame algebra
def _ring_step(y, n):                        # y -> R y, written from VQCSpec.circuit: cx(q, q+1) q = 0..n-2, cx(n-1, 0)
    b = [(y >> q) & 1 for q in range(n)]
    for q in range(n - 1):
        b[q + 1] ^= b[q]
    b[0] ^= b[n - 1]
    return sum(v << q for q, v in enumerate(b))


@pytest.mark.parametrize("n", [9, 12, 16])
def test_ring_frame_algebra(n):
    for y in (1, 5, (1 << n) - 1, 0x5A5 & ((1 << n) - 1), 1 << (n - 1)):
        assert hp.ring_step(y, n) == _ring_step(y, n)
    assert hp.frame_vec(n - 1, 1, n, ring=True) == (1 << (n - 1)) | 3          # the top qubit's vector wraps
    assert hp.frame_rows(1, n, ring=True)[0] == ((1 << n) - 1) & ~1           # row 0 of R is dense
    for k in range(4):
        rows = hp.frame_rows(k, n, ring=True)
        vecs = [hp.frame_vec(q, k, n, ring=True) for q in range(n)]
        for q in range(n):
            for q2 in range(n):
                assert _par(rows[q] & vecs[q2]) == int(q == q2)
            # memory index R^-k e_q holds logical index e_q, and one frame step undoes one ring step
            y = vecs[q]
            for _ in range(k):
                y = _ring_step(y, n)
            assert y == 1 << q
            assert _ring_step(hp.frame_vec(q, k + 1, n, ring=True), n) == vecs[q]


@pytest.mark.parametrize("n", [9, 12, 16])
def test_chain_frames_are_the_old_functions(n):
    def vec(q, k):                           # the chain functions as they were before the ring mode
        v = 1 << q
        for _ in range(k):
            v = (v ^ (v << 1)) & ((1 << n) - 1)
        return v

    def rows(k):
        R = [1 << q for q in range(n)]
        for _ in range(k):
            acc, new = 0, []
            for q in range(n):
                acc ^= R[q]
                new.append(acc)
            R = new
        return R
    for k in range(4):
        assert hp.frame_rows(k, n) == rows(k) == hp.frame_rows(k, n, False)
        assert [hp.frame_vec(q, k, n) for q in range(n)] == [vec(q, k) for q in range(n)]
        g = hp.Group(k + 1, [0, n - 1], k)
        assert g.vecs(n) == [vec(0, k), vec(n - 1, k)] and not g.ring
    none = hp.build_plan(n, 2, [0, 1, 2], False, "ry", tile_bits=8)
    assert not none.ring and none.layer_frame(2) == 0 and none.obs_masks == [1, 2, 4]
    chain = hp.build_plan(n, 2, [0, 1, 2], True, "ry", tile_bits=8)
    assert not chain.ring and chain.layer_frame(2) == 1 and chain.obs_masks == rows(2)[:3]


# ------------------------------------------------------------------------------------------------ plan validity
def _rotations(plan):
    """(layer, q) -> (pass index, position in the execution order, u, r), u and r computed here from the circuit."""
    n = plan.n
    out, pos = {}, 0
    for j, p in enumerate(plan.passes):
        for g in p.groups:
            for q in g.qubits:
                k = g.layer - 1
                u = 1 << q                                   # R^-k e_q by solving R u' = u one step at a time
                for _ in range(k):
                    u = next(v for v in _preimages(u, n))
                cols = []
                for b in range(n):
                    y = 1 << b
                    for _ in range(k):
                        y = _ring_step(y, n)
                    cols.append(y)
                r = sum(((cols[b] >> q) & 1) << b for b in range(n))
                assert (g.layer, q) not in out
                out[(g.layer, q)] = (j, pos, u, r)
            pos += 1
    return out


def _preimages(v, n):
    """The y with R y = v: undo cx(n-1, 0), then the prefix XOR."""
    if (v >> (n - 1)) & 1:
        v ^= 1
    yield (v ^ (v << 1)) & ((1 << n) - 1)


@pytest.mark.parametrize("n,L,t,feat", PROTO + BIG)
def test_ring_plan_is_valid(n, L, t, feat):
    plan = _plan(n, L, t, feat)
    assert plan.ring and not plan.chain and plan.amplitude == (feat == "amplitude")
    rot = _rotations(plan)
    first = plan.first_layer
    assert sorted(rot) == [(l, q) for l in range(first, L + 1) for q in range(n)], "every rotation in exactly one group"
    slots = sorted(s for (l, q) in rot for s in (plan.theta_slot(l, q), plan.theta_slot(l, q) + 1))
    assert slots == list(range(2 * n * (first - 1), plan.n_theta))
    for p in plan.passes:
        assert p.t == plan.t
        for g in p.groups:
            assert g.ring and g.frame == g.layer - 1 == plan.layer_frame(g.layer)
            assert (g.support(n) & ~p.mask()) == 0, "group support leaves its pass tile"
            for q, v in zip(g.qubits, g.vecs(n)):
                assert v == rot[(g.layer, q)][2]
    # every non-commuting pair of rotations runs in layer order (any two layers, not only adjacent ones)
    for a, (_, pa, ua, ra) in rot.items():
        for b, (_, pb, ub, rb) in rot.items():
            if a[0] < b[0] and (_par(ua & rb) or _par(ub & ra)):
                assert pa < pb, f"{b} ran before {a}, which it does not commute with"
    # angle plans: everything run in a pass before owner(q) commutes with the layer-1 rotation of q (u = r = e_q)
    if not plan.amplitude:
        owner = {}
        for j, p in enumerate(plan.passes):
            for g in p.l1:
                for q in g.qubits:
                    assert q not in owner and (p.mask() >> q) & 1
                    assert not any((pp.mask() >> q) & 1 for pp in plan.passes[:j]), "owner is the first tile with q"
                    owner[q] = j
        assert sorted(owner) == list(range(n))
        for o, (j, _, u, r) in rot.items():
            for q in range(n):
                if j < owner[q]:
                    assert not ((u | r) >> q) & 1, f"{o} runs in pass {j}, before layer-1 qubit {q} is measured"
    else:
        assert all(not p.l1 for p in plan.passes)
    # the per-plan kernels derive every address from XOR-linear tables
    codes = set()
    for p, fwd, adj in hp.pass_programs(plan):
        for w in list(fwd) + list(adj):
            code = int(w[hp.W_CODE])
            codes.add(code)
            if code in (hp.OP_OBS, hp.OP_READOUT):
                continue
            tabs = [(hp.W_OFF, 16), (hp.W_BL, 32), (hp.W_BH, 32)] + ([(hp.W_OFF2, 16)] if code in hp.PAIR_CODES else [])
            for base, size in tabs:
                tab = [int(v) for v in w[base:base + size]]
                assert tab[0] == 0
                for i in range(size):
                    assert tab[i] == functools.reduce(lambda x, y: x ^ y, [tab[1 << b] for b in range(5) if (i >> b) & 1 and (1 << b) < size], 0)
                assert all(0 <= v < (1 << p.t) for v in tab)
    assert codes <= {hp.OP_APPLY, hp.OP_APPLY2, hp.OP_BACK, hp.OP_BACK2, hp.OP_GRAD2, hp.OP_GRAD_L1, hp.OP_OBS, hp.OP_READOUT}


def test_ring_pass_counts():
    count = lambda n, L, t=14, f="ry": len(_plan(n, L, t, f).passes)
    assert count(8, 2) == 1 and count(12, 3) == 1 and count(10, 2, 14, "amplitude") == 1     # n <= tile bits
    assert count(16, 2) == 2 and count(20, 2) == 2
    assert count(16, 3) <= 3 and count(16, 3, 14, "amplitude") <= 3
    assert count(24, 3) <= 5
    # (2, 0) does not commute with the layer-1 rotations of qubits >= 1: an angle plan keeps it, and with it all of
    # layer 3, out of pass 0 when the state is larger than the tile
    p16 = _plan(16, 3, 14, "ry")
    assert all(g.layer == 2 and 0 not in g.qubits for g in p16.passes[0].groups)


def test_widened_plan_keeps_the_small_plans_groups():
    small = _plan(16, 3, 13, "ry")
    wide = hp.widen_plan(small, 14)
    sig = lambda pl: [sorted((g.slot, g.layer, tuple(g.qubits), g.frame) for g in p.groups) for p in pl.passes]
    assert sig(wide) == sig(small) and wide.n_slots == small.n_slots and wide.ring and wide.t == 14
    for ps, pw in zip(small.passes, wide.passes):
        assert pw.t == 14 and (pw.mask() & ps.mask()) == ps.mask()
        assert all((g.support(16) & ~pw.mask()) == 0 for g in pw.groups)
    assert sorted(q for p in wide.passes for g in p.l1 for q in g.qubits) == list(range(16))
    # a widened plan computes what the circuit computes: the oracle comparison on a small instance of the same step
    s10 = hp.build_plan(10, 3, _readout(10), feature="ry", tile_bits=8, ring=True)
    w10 = hp.widen_plan(s10, 9)
    ez, gr, x, params, wr, _ = _case(10, 3, "ry")
    ez2, gr2 = hp.emulate(w10, x, params, wr)
    np.testing.assert_allclose(ez2, ez, atol=1e-12)
    np.testing.assert_allclose(gr2, gr, atol=1e-12)


# ------------------------------------------------------------------------------------------------ emulation vs dense
@functools.lru_cache(maxsize=None)
def _case(n, L, feat):
    """Inputs and the dense float64 (complex128) reference of one shape, computed once and shared (read-only)."""
    K, B = (2, 3) if n <= 10 else (1, 2)
    spec = VQCSpec(n, L, 3, feature_map=feat, entangler="ring", readout=_readout(n))
    ops, coef = spec.program()
    prog = TorchProgram(ops, coef, n, dtype=torch.complex128)
    g = torch.Generator().manual_seed(100 * n + L)
    P = spec.n_theta
    params = torch.randn(K, spec.n_params, generator=g, dtype=torch.float64)
    wr = torch.randn(K, B, 3, generator=g, dtype=torch.float64)
    if spec.amplitude:
        raw = torch.randn(K, B, 1 << n, generator=g, dtype=torch.float64)
        raw[0, 0, (1 << n) // 3:] = 0.0
        states = spec.initial_states(raw).to(torch.complex128)
        rows = torch.cat([params[:, None, :P].expand(K, B, P), torch.zeros(K, B, spec.x_width, dtype=torch.float64)],
                         -1).reshape(K * B, -1)
        psi = prog.run(rows, state=states.reshape(K * B, -1))
        x, init = None, states.numpy()
    else:
        xa = torch.rand(K, B, n, generator=g, dtype=torch.float64) * 3
        rows = torch.cat([params[:, None, :P].expand(K, B, P), xa], -1).reshape(K * B, -1)
        psi = prog.run(rows)
        x, init = xa.numpy(), None
    ez = prog.expz(psi, spec.readout).reshape(K, B, -1).numpy()
    gg = prog.adjoint_grads(rows, psi, wr.reshape(K * B, -1), spec.readout)
    gr = slot_grads(gg, prog.ops, prog.coef, rows.shape[1])[:, :P].reshape(K, B, P).sum(1).numpy()
    for a in (ez, gr):
        a.setflags(write=False)
    return ez, gr, x, params.numpy(), wr.numpy(), init


@pytest.mark.parametrize("pair", ["7", "0"])
@pytest.mark.parametrize("n,L,t,feat", PROTO)
def test_emulated_ring_plan_matches_dense(n, L, t, feat, pair, monkeypatch):
    monkeypatch.setenv("QFEDX_HEA_PAIR", pair)
    plan = _plan(n, L, t, feat)
    ez, gr, x, params, wr, init = _case(n, L, feat)
    ez2, gr2 = hp.emulate(plan, x, params, wr, init=init)
    np.testing.assert_allclose(ez2, ez, atol=1e-12)
    np.testing.assert_allclose(gr2, gr, atol=1e-12)


@pytest.mark.parametrize("pair", ["7", "0"])
@pytest.mark.parametrize("n,L,t,feat", [(8, 2, 8, "ry"), (10, 3, 8, "ry"), (12, 3, 10, "amplitude"), (12, 2, 10, "rx")])
def test_emulated_ring_plan_fp16_band(n, L, t, feat, pair, monkeypatch):
    """The kernel's storage format: the bounds of the chain tests (tests/test_hea_plan.py)."""
    monkeypatch.setenv("QFEDX_HEA_PAIR", pair)
    plan = _plan(n, L, t, feat)
    ez, gr, x, params, wr, init = _case(n, L, feat)
    ez3, gr3 = hp.emulate(plan, x, params, wr, fp16=True, init=init)
    print(f"ring fp16 emulation {n}x{L} t{t} {feat}: dZ {np.abs(ez3 - ez).max():.2e} dgrad {np.abs(gr3 - gr).max():.2e}")
    np.testing.assert_allclose(ez3, ez, atol=2e-3)
    np.testing.assert_allclose(gr3, gr, atol=3e-3 * max(1.0, np.abs(gr).max()))


# ------------------------------------------------------------------------------------------------ chain plans untouched
# sha256 over every pass's forward ops, adjoint ops and their fo_tables, computed on the commit before the ring mode
CHAIN_DIGESTS = {
    (16, 3, True, "ry"): "a79cfc78435e47c540ef4b3e2db51ca70e309f04d15decfb479bcb6881eb1c3f",
    (20, 2, True, "ry"): "1289f6dee36bbf17f3100daf90747283686ce965082ec6ac9a1f3178c4951976",
    (24, 3, True, "ry"): "d27bc8cc5c1558dac43198b65c17fabe8fe54fe1227673bdd1b04e4e5736fe1f",
    (10, 3, True, "amplitude"): "f876d5367a1816e0faf7cd21a877181ebd0887107669de4903b3f048ec056acb",
    (16, 3, True, "amplitude"): "749fa321bccb5cd7f11c67b7d448cca214ffb186136eb4d752c133ef5ad47de6",
    (12, 2, False, "ry"): "0988a0698264b602552eb48dbe230ae67380bd52ae133d1ede8b2eecdd935f78",
}


@pytest.mark.parametrize("case", sorted(CHAIN_DIGESTS, key=str))
def test_chain_plans_are_bitwise_what_they_were(case, monkeypatch):
    monkeypatch.delenv("QFEDX_HEA_PAIR", raising=False)
    n, L, chain, feat = case
    hp._PLAN_CACHE.pop((n, L, (0, 1, 2), chain, feat, hp.TILE_BITS, True), None)
    _plan(n, L, hp.TILE_BITS, feat)                     # a ring plan of the same shape must not leak into the chain's
    plan = hp.build_plan(n, L, [0, 1, 2], chain, feat)
    h = hashlib.sha256()
    for p, f, a in hp.pass_programs(plan):
        h.update(np.ascontiguousarray(f, dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(hp.fo_table(f, p, n)).tobytes())
        h.update(np.ascontiguousarray(hp.fo_table(a, p, n)).tobytes())
    assert h.hexdigest() == CHAIN_DIGESTS[case]


# ------------------------------------------------------------------------------------------------ routing
def test_ring_routing_and_eligibility():
    spec = VQCSpec(16, 3, 3, entangler="ring")
    assert hp.eligible_ring(spec) and not hp.eligible(spec) and not hp.eligible_amplitude(spec)
    amp = VQCSpec(10, 2, 3, feature_map="amplitude", entangler="ring")      # planned and emulated, not run: refused
    assert not hp.eligible_ring(amp) and not hp.eligible_amplitude(amp) and "amplitude" in hp.refusal(amp)
    assert not hp.eligible_ring(VQCSpec(16, 3, 3)) and not hp.eligible_ring(VQCSpec(16, 3, 3, entangler="none"))
    assert resolve_state_dtype("auto", spec, "hip", None) == "fp32"
    assert resolve_state_dtype("bf16", spec, "hip", None) == "bf16"
    for explicit in ("mfma", "fp16", "mfma_bf16"):
        assert resolve_state_dtype(explicit, spec, "hip", None) == explicit
    assert hp.refusal(spec) == ""
    for bad, word in ((VQCSpec(16, 3, 3, entangler="ring", noisy=True), "gate noise"),
                      (VQCSpec(7, 2, 3, entangler="ring"), "7 qubits"),
                      (VQCSpec(10, 2, 9, entangler="ring"), "9 classes")):
        assert not hp.eligible_ring(bad)
        assert word in hp.refusal(bad)


def test_ring_plan_call_forms_and_cache():
    a = hp.build_plan(10, 2, [0, 1, 2], feature="ry", tile_bits=8, ring=True)
    b = hp.build_plan(10, 2, [0, 1, 2], "ring", "ry", tile_bits=8)
    c = hp.build_plan(10, 2, [0, 1, 2], True, "ry", tile_bits=8)
    assert a.ring and b.ring and not c.ring and c.chain
    sig = lambda pl: [(p.c, p.lo, p.hi, [(g.layer, tuple(g.qubits)) for g in p.groups]) for p in pl.passes]
    assert sig(a) == sig(b) and a.obs_masks != c.obs_masks
    assert (10, 2, (0, 1, 2), False, "ry", 8, True, "ring") in hp._PLAN_CACHE
    with pytest.raises(ValueError):
        hp.build_plan(2, 2, [0, 1], ring=True)
