"""CPU tests that pin the pass planner's output and its forward / adjoint plan choice (``hea_plan.plan_pair``): digests
of whole plans (tile geometry, swizzle rows, groups, layer-1 groups and every table the kernels read) for chain,
no-entangler, ring, widened, small-tile and amplitude plans, and the decision tree ``HeaMfmaProgram`` runs its plans
through.  None of them needs the native extension."""
import hashlib

import numpy as np
import pytest

from qfedx_amd.ops import hea_plan as hp

READOUT = [0, 1, 2]

# (entangler, feature, n, L, tile bits, widened to): sha256 of ``_digest``, computed on the commit before the chain and
# ring planners were merged into one loop
DIGESTS = {
    ("ring", "ry", 8, 2, 8, None): "3ef4e266751265f7e8eb448b8061edf99fbaadd7b44b85f59638c3ede4ec97b5",
    ("ring", "ry", 10, 3, 8, None): "567173f8b75f832ae6b8e1ddb7a2615eab2401a3ab262426ed1ced1d6b8449a4",
    ("ring", "ry", 12, 2, 10, None): "b552b31825e5facf62cf87d5b9f0a662d42b29620d68da16443ca01a61fceb32",
    ("ring", "ry", 16, 3, 13, None): "765f974c61bf93e1b57f123b223bf30126779d95d112ee6501eeeb82de6494db",
    ("ring", "ry", 16, 3, 14, None): "0855357a1ddca2d1a8a7dc1f21d925bc8f386e795f0af1ccedfbd665ad8d469b",
    ("ring", "ry", 24, 3, 14, None): "21d29fba5520489f0f724b6e43fb31396f5703636279879b93df5f86e10e4ba7",
    ("ring", "amplitude", 10, 2, 8, None): "59f7bd6a485d15f994ad3250ac161b33d47fbcf3611f8bb9637c44881ce5ce20",
    ("ring", "ry", 10, 3, 8, 14): "b187a3703a7c978802cfea9022f332cced97159b7f700ba877f0bc9f62d080a2",
    ("ring", "ry", 12, 2, 10, 14): "aafe7207c506c3c4e5f6bb2a00b4ce9aa8697d1912612984a2e0052d26f3a504",
    ("ring", "ry", 16, 3, 13, 14): "53f887c132e259d4a049a82990584b2a8b67583decdf555e7c160505fba9e83a",
    ("chain", "ry", 16, 3, 13, None): "bcba70aacece978d6f9be40dc358671fab661917d4cd3fc31b73e6388119c603",
    ("chain", "amplitude", 12, 2, 10, None): "3bf60d06ccfc1f28018c0d00cd6c0db7cc6a19770dfca2100a0059debbe89b9e",
    # L = 1 angle plans place no rotation: chain = pass 0 and a coverage pass, ring = coverage passes only
    ("chain", "ry", 16, 1, 14, None): "d0917f57f62bb18033d7c10d844a54d07d62f34d7793f96f6ad44e6609466673",
    ("none", "ry", 12, 2, 8, None): "19b2a977667c33ced75c6c7d701248c24149867f5ec0661a0de2c0532f9c861f",
    ("ring", "ry", 8, 1, 8, None): "3fa0427b383c3793af4075845506c0e35055deda862aae9a3d6f42f919a49d96",
    ("ring", "ry", 16, 1, 14, None): "e983e71927eb4bab28ebe3fb520a44f35dea1d1f9e0634150b6ce61c0e882bf0",
}


def _groups(gs):
    return [(g.layer, tuple(g.qubits), g.frame, g.slot, g.ring) for g in gs]


def _digest(plan) -> str:
    h = hashlib.sha256()
    h.update(repr((plan.n, plan.L, plan.C, plan.readout, plan.chain, plan.ring, plan.feature, plan.t,
                   plan.n_slots)).encode())
    for p, f, a in hp.pass_programs(plan):
        h.update(repr((p.c, p.lo, p.hi, [int(x) for x in p.H], _groups(p.groups), _groups(p.l1))).encode())
        h.update(np.ascontiguousarray(f, dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
        h.update(np.ascontiguousarray(hp.fo_table(f, p, plan.n)).tobytes())
        h.update(np.ascontiguousarray(hp.fo_table(a, p, plan.n)).tobytes())
    return h.hexdigest()


def _evict(ent, feat, n, L, t, wide):
    """Drop the case's cached plan - a widened case's: every widening of its shape to that size; its source plan is a
    case of its own - so that the next call plans it."""
    if wide is None:
        hp._PLAN_CACHE.pop((n, L, tuple(READOUT), ent == "chain", feat, t, True) + (("ring",) if ent == "ring" else ()), None)
    for key in [k for k in hp._PLAN_CACHE if k[:3] == ("widen", n, L) and k[7] == wide]:
        del hp._PLAN_CACHE[key]


def _build(ent, feat, n, L, t):
    return hp.build_plan(n, L, READOUT, ent == "chain", feat, tile_bits=t, ring=ent == "ring")


@pytest.mark.parametrize("case", list(DIGESTS), ids=str)
def test_plans_are_bitwise_what_they_were(case, monkeypatch):
    monkeypatch.delenv("QFEDX_HEA_PAIR", raising=False)
    ent, feat, n, L, t, wide = case
    _evict(*case)
    plan = _build(ent, feat, n, L, t)
    if wide is not None:
        plan = hp.widen_plan(plan, wide)
        assert plan.t == min(wide, n)
    assert plan.ring == (ent == "ring") and plan.chain == (ent == "chain")
    assert _digest(plan) == DIGESTS[case]


def test_ring_plan_without_rotations_has_no_pass_zero():
    """An L = 1 angle plan places no rotation: the chain plan still opens with pass 0, the ring plan's tiles come from
    the coverage loop alone."""
    tiles = lambda pl: [(p.c, p.lo, p.hi) for p in pl.passes]
    assert tiles(_build("ring", "ry", 8, 1, 8)) == [(5, 5, 8)]
    ring = _build("ring", "ry", 16, 1, 14)
    assert len(ring.passes) == 2 and all(p.hi > p.lo for p in ring.passes)
    chain = _build("chain", "ry", 16, 1, 14)
    assert tiles(chain)[0] == (14, 14, 14) and len(chain.passes) == 2
    assert all(not p.groups for pl in (ring, chain) for p in pl.passes)


# ------------------------------------------------------------------------------------------------ plan pairs
PAIRS = [("chain", "ry", 16, 3, 14, 13, True), ("ring", "ry", 16, 3, 14, 13, True),
         ("ring", "ry", 16, 3, 14, 13, False), ("ring", "ry", 16, 3, 14, 14, True),
         ("chain", "amplitude", 12, 2, 10, 8, True), ("none", "ry", 12, 2, 8, 8, True),
         ("ring", "ry", 10, 3, 14, 8, True), ("ring", "ry", 12, 2, 10, 8, True), ("chain", "ry", 16, 1, 14, 13, True)]


def _pair(ent, feat, n, L, t, ta, from_adj):
    return hp.plan_pair(n, L, READOUT, ent, feat, t, ta, from_adj)


def test_chain_pair_runs_the_adjoint_on_small_tiles():
    fwd, adj = _pair("chain", "ry", 16, 3, 14, 13, True)
    assert fwd.t == 14 and adj.t == 13 and all(p.t == 13 for p in adj.passes)
    assert hp.same_passes(fwd, adj)
    assert _digest(fwd) == _digest(_build("chain", "ry", 16, 3, 14))
    assert _digest(adj) == _digest(_build("chain", "ry", 16, 3, 13)) == DIGESTS[("chain", "ry", 16, 3, 13, None)]


def test_ring_pair_widens_the_small_plan_for_the_forward(monkeypatch):
    monkeypatch.delenv("QFEDX_HEA_PAIR", raising=False)
    fwd, adj = _pair("ring", "ry", 16, 3, 14, 13, True)
    small = _build("ring", "ry", 16, 3, 13)
    assert not hp.same_passes(_build("ring", "ry", 16, 3, 14), small), "the case must reach the widening branch"
    assert adj.t == 13 and _digest(adj) == _digest(small)
    assert fwd.t == 14 and _digest(fwd) == _digest(hp.widen_plan(small, 14)) == DIGESTS[("ring", "ry", 16, 3, 13, 14)]
    assert hp.same_passes(fwd, adj)


def test_ring_pair_keeps_its_own_forward_plan_when_asked():
    fwd, adj = _pair("ring", "ry", 16, 3, 14, 13, False)
    assert adj is fwd and fwd.t == 14
    assert _digest(fwd) == _digest(_build("ring", "ry", 16, 3, 14))


@pytest.mark.parametrize("ent", ["chain", "ring"])
def test_equal_tile_sizes_share_one_plan(ent):
    fwd, adj = _pair(ent, "ry", 16, 3, 14, 14, True)
    assert adj is fwd and _digest(fwd) == _digest(_build(ent, "ry", 16, 3, 14))


@pytest.mark.parametrize("case", PAIRS, ids=str)
def test_every_pair_has_the_same_passes(case):
    fwd, adj = _pair(*case)
    assert hp.same_passes(fwd, adj) and fwd.n_slots == adj.n_slots
    assert len(fwd.passes) == len(adj.passes)
    assert fwd.ring == adj.ring == (case[0] == "ring") and fwd.chain == adj.chain == (case[0] == "chain")


def test_a_widened_plan_that_lost_a_group_is_refused(monkeypatch):
    def lossy(plan, tile_bits, swizzle=True):
        return hp.build_plan(plan.n, plan.L, plan.readout, plan.chain, plan.feature, tile_bits, ring=plan.ring)
    monkeypatch.setattr(hp, "widen_plan", lossy)
    with pytest.raises(RuntimeError, match="lost a group"):
        _pair("ring", "ry", 16, 3, 14, 13, True)
