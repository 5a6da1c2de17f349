"""MFMA statevector engine for the hardware-efficient VQC (host side).

``HeaMfmaProgram`` runs the pass plans of ``ops/hea_plan.py`` on the gfx950 kernels of
``csrc/hea_mfma.hip``: per local step

    hea_frags (per-client 16 x 16 group unitaries -> MFMA A fragments, hi + lo fp16)
    forward passes  (product state generated in-tile; intermediate pass outputs stored as fp16 (re, im))
    readout_ce      (shared with the VALU engine: <Z>, CE loss, dL/d<Z>, a/b gradients; noiseless steps instead
                     compute them per sample in hea_readout_rec or inside the last adjoint pass: ``readout_mode``)
    adjoint passes  (reverse pass order; per-workgroup gradient partials)
    hea_grad_reduce (fixed-order sum over each client's samples and tiles)

Every pass, forward or adjoint, of every route (training step, DP-SGD step, ``expz``, ``vjp``, the parameter-shift
branches) is launched by ``HeaMfmaProgram._launch``, which derives the kernel's flags from the buffers it is given.
What the host launches is pinned without a GPU: tools/hea_launch_trace.py records every native call with its arguments
(workspaces by name, pass tables by identity) and tests/test_hea_launch_trace.py compares them, and the sha256 of every
table the constructor builds, with tests/golden/hea_launch_traces.json.

It exposes the subset of ``HipProgram``'s interface the engine / trainer use (``expz``, ``vjp``,
``loss_and_grads``, ``private_workspace``), so ``VQCEngine(..., backend="hip", state_dtype="mfma")``
swaps it in for circuits ``hea_plan.eligible`` accepts.  Amplitude-encoded circuits (``hea_plan.eligible_amplitude``)
run too: real ``init`` rows are normalised and written in the storage format by ``hea_amp_stage`` (csrc/hea_amp.hip),
forward pass 0 loads that buffer instead of generating a product state, and layer 1 is an ordinary rotation layer of
the plan.  Ring-entangler circuits (``hea_plan.eligible_ring``) run on ring plans (``build_plan(ring=True)``): the same
kernels, other tables.  Amplitudes are stored as fp16 scaled by
2^(n/2) (unit-magnitude typical values); MFMAs accumulate in fp32 and the unitaries carry a hi/lo fp16
split, so the only rounding is the fp16 state between ops (~2^-12 relative per op).
"""
from __future__ import annotations

import contextlib
import os
from collections import namedtuple

import numpy as np
import torch

from ._ext import ext
from .hea_plan import (OP_APPLY, OP_APPLY2, OP_BACK, OP_BACK2, OP_GRAD2, OP_GRAD_L1, OP_READOUT, TILE_BITS, W_CODE, W_SLOT,
                       W_SLOT2, eligible, eligible_amplitude, eligible_ring, fo_table, obs_table, pass_programs, plan_pair,
                       refusal)

ADJ_TILE_BITS = 13   # adjoint tiles: 2^13 amplitudes x (psi, lambda) = 64 KB of LDS -> two workgroups per CU

_FEATURE = {"ry": 0, "rx": 1, "rz": 2, "amplitude": 0}      # (an amplitude program never generates: unused)


def _frag_index(ops: np.ndarray) -> torch.Tensor:
    """Per op the unitary fragments it multiplies by (slot * 4 + 0: U, + 2: U^H; a pair op names its two groups'),
    -1 for none: int32 [nops, 2] (prefetch table)."""
    out = np.full((len(ops), 2), -1, dtype=np.int32)
    for i, w in enumerate(ops):
        code = int(w[W_CODE])
        if code in (OP_APPLY, OP_APPLY2):
            out[i, 0] = 4 * int(w[W_SLOT])
        elif code in (OP_BACK, OP_BACK2):
            out[i, 0] = 4 * int(w[W_SLOT]) + 2
        if code == OP_APPLY2:
            out[i, 1] = 4 * int(w[W_SLOT2])
        elif code == OP_BACK2:
            out[i, 1] = 4 * int(w[W_SLOT2]) + 2
    return torch.from_numpy(out).contiguous()


def _knob(name: str, unset, on: str | None = None):
    """Environment knob ``name``: ``unset`` while unset or empty, else whether it is not ``0`` (``on``: is that value)."""
    env = os.environ.get(name, "")
    return unset if env == "" else (env == on if on is not None else env != "0")


def spec_default() -> bool:
    """Per-plan pass kernels (csrc/hea_spec.cpp) instead of the interpreter: on by default, ``QFEDX_HEA_SPEC=0`` selects
    the interpreter (docs/ARCHITECTURE.md section 1b).  ``QFEDX_DEBUG=1`` stays on the interpreter: the device checks
    validate the op records the per-plan build no longer reads."""
    return os.environ.get("QFEDX_DEBUG", "0") != "1" and _knob("QFEDX_HEA_SPEC", True)


def split_readout_default():
    """``QFEDX_HEA_SPLIT_RO`` = 1 / 0 forces the split-readout step on / off wherever it is possible
    (``HeaMfmaProgram.readout_mode``); unset (None): by sample count, ``SPLIT_READOUT_MIN_SAMPLES``.  ``0`` makes every
    step launch what it launched before the split route existed."""
    return _knob("QFEDX_HEA_SPLIT_RO", None)


def obs_load_default() -> bool:
    """``QFEDX_HEA_OBS_LOAD`` = 1 / 0: the per-plan kernel of the last adjoint pass seeds lambda while it loads its
    tile and runs no observable op (csrc/hea_mfma.hip seed_tile_il) / keeps the op, i.e. compiles exactly the text it
    compiled before the seeding load existed.  Read when a program is built (``HeaMfmaProgram.obs_at_load``)."""
    return _knob("QFEDX_HEA_OBS_LOAD", OBS_LOAD_DEFAULT)


def spec_gen_default(unset: bool = False) -> bool:
    """``QFEDX_HEA_SPEC_GEN`` = 1 / 0: the forward pass that generates the layer-1 product state (pass 0 of an angle
    program) gets a per-plan kernel like every other pass / stays on the interpreter.  Both generate the same bits: the
    per-plan build writes the generation's fp32 products with the interpreter's roundings (csrc/hea_common.h cmul_pin).  Read when a program is built
    (``HeaMfmaProgram.spec_gen``); amplitude programs have no such pass.  Unset, the caller decides (``unset``): the
    engine (ops/engine.py: training, evaluation, the benchmark) turns it on, ``SPEC_GEN_ENGINE``; a program built
    directly keeps pass 0 on the interpreter unless it is asked (``spec_gen=True``), as ``spec_passes()`` has always
    reported it for such a program."""
    return _knob("QFEDX_HEA_SPEC_GEN", bool(unset))


def spec_lean_default(unset: int = 0) -> int:
    """``QFEDX_HEA_SPEC_LEAN`` = a bit mask, 0..7: work the per-plan kernels leave out (csrc/hea_spec.h ``HEA_LEAN_*``).
    1: adjoint pair ops hold the im-row fragments of their op instead of re-deriving them per block; 2: no op barrier
    between two gradient ops that only read the tile; 4: a pass's tile store is issued ahead of a read-only tail (the
    readout of a forward pass, trailing cross-only gradient ops of an adjoint pass).  Every part gives bitwise the same
    results, and ``0`` compiles exactly the text of before the knob.  Read when a program is built
    (``HeaMfmaProgram.spec_lean``).  Unset, the caller decides (``unset``): the engine turns on ``SPEC_LEAN_ENGINE``,
    a program built directly keeps 0 unless it is asked (``spec_lean=``)."""
    env = os.environ.get("QFEDX_HEA_SPEC_LEAN", "")
    mask = int(unset) if env == "" else int(env)
    if not 0 <= mask <= 7:
        raise ValueError(f"QFEDX_HEA_SPEC_LEAN must be a bit mask 0..7, got {mask}")
    return mask


def ring_fwd_from_adj() -> bool:
    """``QFEDX_HEA_RING_ADJ`` = 13 / 14: a ring program's forward runs the groups of its 2^13-tile plan on widened
    tiles, so the adjoint runs on 2^13 tiles (two workgroups per CU) / the forward runs its own 2^14 plan (fewer group
    ops) and the adjoint runs on the same 2^14 tiles.  Default ``RING_FWD_FROM_ADJ``."""
    return _knob("QFEDX_HEA_RING_ADJ", RING_FWD_FROM_ADJ, on="13")


_SPEC_WARNED = False
_NO_KEYS = torch.zeros(0, dtype=torch.int64)
_NODBG = torch.zeros(0, dtype=torch.int64)     # no stall-attribution buffer (stamps build only)


NT_STORE_MIN_BYTES = 128 << 20   # pass states above which tiles are stored non-temporally (_nt_store)
FUSED_ADAM_MAX_BLOCKS = 256   # hea_grad_reduce blocks (clients x gradient ops) up to which Adam is fused
# Samples per step (clients x batch) from which a noiseless step computes the readout records in a launch of their own
# and runs the last adjoint pass per plan (readout_mode).  Measured, 16q x 3L, clients x 32 samples, ms per round fused
# -> split: 32 samples 0.090 -> 0.089 and 64 samples 0.111 -> 0.109 (inside 3 x the run-to-run spread), 128 samples
# 0.166 -> 0.159, 256 0.270 -> 0.253, 512 0.480 -> 0.444, 2048 1.659 -> 1.509 (profiles/split_readout_ab.txt).  Never
# below 64: steps of a few samples stay fused whatever a box measures.
SPLIT_READOUT_MIN_SAMPLES = 128
# The per-plan last adjoint pass seeds lambda during its tile load (obs_load_default): bitwise the same results.
# Measured, 16q x 3L, clients x 32 samples, ms per round parent -> knob 1, two boxes (profiles/obs_at_load_ab.txt):
# 64 clients 1.589 -> 1.555 (3 x the parent's spread: 0.036, missed by 0.001) and 1.684 -> 1.663 (0.012, met), every
# knob-1 run below every parent run; 8 clients 0.255 -> 0.250, inside three spreads (0.016): a tie.  Compiled into the
# one kernel a pass has, so not gated by sample count.
OBS_LOAD_DEFAULT = True
# The engine's programs run the generating forward pass per plan (spec_gen_default): bitwise the same results.
# Measured, 16q x 3L, clients x 32 samples, ms per round parent -> knob 1, alternating x 3 on one box
# (profiles/hea_spec_gen_ab.txt): 64 clients 1.583 -> 1.539 (3 x the parent's spread: 0.024, met; pass 0 itself 0.30 ->
# 0.265 ms per dispatch); 8 clients 0.254 -> 0.247, inside three spreads (0.015).
SPEC_GEN_ENGINE = True
# The engine's programs compile their per-plan kernels with the held im-row fragments (spec_lean_default, part 1):
# bitwise the same results.  Measured, 16q x 3L, clients x 32 samples, ms per round parent -> mask 1, alternating on one
# box, two boxes (profiles/hea_spec_lean_ab.txt): 64 clients 1.526 -> 1.497 (3 x the parent's spread: 0.006) and 1.491
# -> 1.468 (0.021), every mask-1 run below every parent run; the adjoint passes 0.604 -> 0.583 and 0.422 -> 0.409 ms per
# dispatch; 8 clients 0.246 -> 0.240.  Parts 2 (no barrier between cross-only gradient ops) and 4 (tile stores ahead of
# a read-only tail) did not hold their own - alone 1.526 -> 1.527 and 1.522, and part 4 slowed the pass that stores
# lambda (0.422 -> 0.430 ms: the store's cost is its issue, LDS reads included, not its drain) - and stay off.
SPEC_LEAN_ENGINE = 1
# Ring programs: forward on the 2^13 plan's grouping with a 2^13 adjoint (True) or native 2^14 groups with a 2^14
# adjoint (False); 16q x 3L: 9 against 8 group ops, both in 3 passes.  Measured, clients x 32 samples, ms per step,
# alternating x 3 on one box (profiles/hea_ring_plan_ab.txt): 64 clients 2.070 -> 2.021 (every run below every native
# run), 8 clients 0.339 -> 0.332: the pass with the layer-1 gradient groups gains more from two workgroups per CU
# (0.52 -> 0.40 ms) than the extra group op costs the other passes.
RING_FWD_FROM_ADJ = True


# passes[j] = (the forward plan's pass, its device tables, the adjoint program's tables, the adjoint plan's pass), tables =
# (op records, per-op fragment prefetch indices, fragment-order table): tuples, so indexing and unpacking them works too
PassTables = namedtuple("PassTables", "ops fidx fo")
PassEntry = namedtuple("PassEntry", "fwd_pass fwd adj adj_pass")
# what every pass launch of one host call takes: inputs, parameter rows, fragments, clients, batch, whether the fragments
# are one shared set, the stamps build's per-pass buffers (stamp_buffers) or None
_Call = namedtuple("_Call", "x params fr K B shared dbg")


class HeaMfmaProgram:
    def __init__(self, spec, device, tile_bits: int | None = None, adj_tile_bits: int | None = None,
                 storage: str = "fp16", use_spec: bool | None = None, spec_gen: bool | None = None,
                 spec_lean: int | None = None):
        """``storage``: fp16 (default) or bf16 (BASELINE config 2) amplitudes and unitary fragments
        (csrc/hea_mfma_bf16.hip: v_mfma_f32_16x16x32_bf16, fp32 accumulation; 2^-9 per-op state rounding)."""
        if storage not in ("fp16", "bf16"):
            raise ValueError(f"MFMA engine storage must be fp16 | bf16, got {storage!r}")
        self.storage = storage
        self.bf16 = storage == "bf16"
        if not (eligible(spec) or eligible_amplitude(spec) or eligible_ring(spec)):
            raise ValueError("the MFMA engine covers angle-encoded (hea_plan.eligible) and amplitude-encoded "
                             "(hea_plan.eligible_amplitude) RX/RZ + CNOT-chain VQCs and angle-encoded ring-entangler "
                             "ones (hea_plan.eligible_ring) with 8..30 qubits, no gate noise and <= 8 classes; refused: "
                             + refusal(spec))
        self.spec = spec
        # ring entangler: the plans' frames count ring layers (hea_plan.frame_vec(ring=True)); the kernels are table
        # driven and run them unchanged
        self.ring = spec.entangler == "ring"
        # amplitude program: forward pass 0 loads the staged input states (``_stage``) instead of generating the
        # layer-1 product state, and every layer's rotations are group ops
        self.amplitude = bool(spec.amplitude)
        self.n = spec.n_qubits
        self.C = spec.n_classes
        self.n_theta = spec.n_theta
        self.device = torch.device(device)
        if tile_bits is None:
            tile_bits = int(os.environ.get("QFEDX_HEA_TILE", TILE_BITS))
        if adj_tile_bits is None:
            adj_tile_bits = int(os.environ.get("QFEDX_HEA_ADJ_TILE", min(tile_bits, ADJ_TILE_BITS)))
        self.tile_bits = tile_bits
        # the adjoint runs on its own (smaller) tiles where a plan with the forward's passes exists: hea_plan.plan_pair
        self.plan, plan_a = plan_pair(self.n, spec.n_layers, spec.readout, spec.entangler, spec.feature_map, tile_bits,
                                      adj_tile_bits, ring_fwd_from_adj())
        self.adj_plan = plan_a
        self.adj_tile_bits = plan_a.passes[0].t if plan_a.passes else tile_bits
        self.n_slots = self.plan.n_slots
        self._lower_plans()
        self._build_slot_table()
        self.slab_tiles = max(1 << (self.n - p.t) for p in plan_a.passes)
        self.scale = float(1 << (self.n // 2))
        self.feature = _FEATURE[spec.feature_map.lower()]
        self._iempty = torch.empty(0, dtype=torch.int32, device=self.device)      # "no buffer" of a launch
        self._fempty = torch.empty(0, dtype=torch.float32, device=self.device)
        self._ws = {}
        self._ps_budget = None
        if self.device.type == "cuda":
            self._shift_budget()      # query free HBM now, never inside a graph capture
        # noiseless steps compute the readout in the first adjoint pass (profiles/r5_fused_readout_ab.txt: a tie at 64
        # clients, -2.7% at 8); the readout kernel runs for readout noise - and for tests comparing the two (False).
        # Larger steps compute the same values in a launch of their own ahead of the adjoint (readout_mode: split).
        self.fused_readout = True
        # knobs, read when the program is built.  Per-plan pass kernels or the interpreter:
        self.spec_requested = spec_default() if use_spec is None else bool(use_spec)
        # split-readout steps (readout_mode): None = by sample count, True / False = wherever possible / never
        self.split_readout = split_readout_default()
        # the per-plan kernel of a pass that starts with the observable op seeds lambda in its tile load (spec_cfg)
        self.obs_at_load = obs_load_default()
        # the pass that generates the layer-1 product state gets a per-plan kernel too (False: the interpreter)
        self.spec_gen = spec_gen_default() if spec_gen is None else bool(spec_gen)
        # work the per-plan kernels leave out, a bit mask (0: the kernels of before the knob)
        self.spec_lean = spec_lean_default() if spec_lean is None else int(spec_lean)
        # per-plan pass kernels: compiled (or loaded from the cache) and their modules loaded here, never inside a
        # stream capture
        self.spec_fwd, self.spec_adj, self.spec_keys = [-1] * self.n_passes, [-1] * self.n_passes, []
        self.spec_launches = self.interp_launches = 0      # pass launches that ran a per-plan kernel / the interpreter
        if self.spec_requested:
            self.prepare_spec()

    def _lower_plans(self) -> None:
        """Both plans -> per-pass programs and tables: ``passes``, ``_host_progs``, ``n_regions``, ``fwd_last``,
        ``gmeta`` / ``n_gradops`` / ``grad_cover_exact``; every program is checked on the host (``hea_check_ops``)."""
        gmeta = []
        progs_f = pass_programs(self.plan, [])
        progs_a = pass_programs(self.adj_plan, gmeta)
        # Forward passes after the last one that applies a unitary are identities on the state (they exist for
        # the adjoint's layer-1 gradient tiles, e.g. every pass of an L = 1 circuit): the forward stops at that
        # pass, reads out there, and later passes' stored outputs alias its output.
        applies = [j for j, (_, fwd, _) in enumerate(progs_f)
                   if any(int(w[W_CODE]) in (OP_APPLY, OP_APPLY2) for w in fwd)]
        self.fwd_last = R = applies[-1] if applies else 0
        if R < len(progs_f) - 1:
            pr, fr_ops, _ = progs_f[R]
            fr_ops = np.concatenate([fr_ops, obs_table(self.plan, pr, OP_READOUT)[None]], 0)
            progs_f = [(p, f if j < R else (fr_ops if j == R else f[:0]), a) for j, (p, f, a) in enumerate(progs_f)]
        self.n_gradops = len(gmeta)
        self.gmeta = torch.tensor(gmeta, dtype=torch.int32).reshape(-1).to(self.device)
        # the fused Adam epilogue of hea_grad_reduce updates each parameter in the block that formed its gradient:
        # it needs every theta parameter owned by exactly one gradient record (else the separate Adam launch runs)
        owned = []
        for row in gmeta:
            nr = int(row[1]) & 15
            owned += [int(v) for v in row[2:2 + nr]] + [int(v) for v in row[6:6 + nr]]
        self.grad_cover_exact = sorted(owned) == list(range(self.n_theta))
        self.passes = []
        self.n_regions = []       # per pass: gradient records of its adjoint program (LDS regions)
        self._host_progs = []     # per pass: host (ops, fidx) of the forward / adjoint programs (per-plan kernels)

        def tables(ops, p, adjoint):
            t, fidx = torch.from_numpy(ops.astype(np.int32)).contiguous(), _frag_index(ops)
            ext().hea_check_ops(t, fidx, self.n_slots, self.n_theta, adjoint, p.t, self.n_gradops)
            fo = torch.from_numpy(fo_table(ops, p, self.n).reshape(-1))
            return (t, fidx), PassTables(t.to(self.device), fidx.to(self.device), fo.to(self.device))
        for (p, fwd, _), (pa, _, adj) in zip(progs_f, progs_a):
            (hf, df), (ha, da) = tables(fwd, p, False), tables(adj, pa, True)
            self.n_regions.append(sum(2 if int(w[W_CODE]) in (OP_BACK2, OP_GRAD2) else
                                      int(int(w[W_CODE]) in (OP_BACK, OP_GRAD_L1)) for w in adj))
            self.passes.append(PassEntry(p, df, da, pa))
            self._host_progs.append((hf, ha))

    def _build_slot_table(self) -> None:
        """``slot_tab``: per unitary slot its qubit count and the theta indices of its rotations (hea_frags); every
        parameter must be owned by a pass."""
        slot_tab = np.zeros((max(self.n_slots, 1), 9), dtype=np.int32)
        owner = np.zeros(self.n_theta, dtype=np.int32)
        for p in self.plan.passes:
            nt = 1 << (self.n - p.t)
            for g in p.groups:
                slot_tab[g.slot, 0] = len(g.qubits)
                for j, q in enumerate(g.qubits):
                    slot_tab[g.slot, 1 + j] = self.plan.theta_slot(g.layer, q)
                    slot_tab[g.slot, 5 + j] = self.plan.theta_slot(g.layer, q) + 1
            for g in p.groups + p.l1:
                for q in g.qubits:
                    owner[self.plan.theta_slot(g.layer, q)] = nt
                    owner[self.plan.theta_slot(g.layer, q) + 1] = nt
        if (owner == 0).any():
            raise RuntimeError("a parameter has no owning pass")
        self.slot_tab = torch.from_numpy(slot_tab).to(self.device)

    @property
    def spec_active(self) -> bool:
        """At least one pass of this program has a per-plan kernel.  Which passes a step launches per plan:
        ``spec_passes``; how many launches actually did: ``spec_launches`` / ``interp_launches``."""
        return any(h >= 0 for h in self.spec_fwd + self.spec_adj)

    def readout_mode(self, samples: int | None = None, noise=None) -> str:
        """How a training step of ``samples`` samples (clients x batch) computes its readout:

        ``kernel``  the readout / cross-entropy kernel (readout noise, ``fused_readout`` off, > 64 partials per sample)
        ``fused``   inside the last adjoint pass, which therefore runs on the interpreter (``_adj_handle``)
        ``split``   ``hea_readout_rec`` writes every sample's <Z>, dL/d<Z> and reduction record once, bitwise what the
                    fused pass writes, and the last adjoint pass runs its per-plan kernel: chosen among the steps that
                    would fuse when that pass has a per-plan kernel and ``samples >= SPLIT_READOUT_MIN_SAMPLES``
                    (``split_readout`` = True / False replaces the sample-count rule).
        Without a sample count: ``fused`` or ``kernel``, the meaning ``spec_passes()`` always had."""
        if not self._fused_readout(noise):
            return "kernel"
        if samples is None or not self.spec_adj or self.spec_adj[-1] < 0:
            return "fused"
        split = samples >= SPLIT_READOUT_MIN_SAMPLES if self.split_readout is None else self.split_readout
        return "split" if split else "fused"

    def spec_passes(self, fused_readout: bool | None = None, samples: int | None = None) -> dict:
        """Per pass, whether a training step launches its per-plan kernel (True) or the interpreter: forward passes
        0..fwd_last and adjoint passes 0..J-1.  ``fused_readout`` (default: what a noiseless step does): the last
        adjoint pass then runs on the interpreter - unless the step has ``samples`` samples and takes the split route
        (``readout_mode``)."""
        fused = self._fused_readout(None) if fused_readout is None else fused_readout
        if fused and samples is not None and self.readout_mode(samples) == "split":
            fused = False
        J = self.n_passes
        return {"fwd": [self.spec_fwd[j] >= 0 for j in range(self.fwd_last + 1)],
                "adj": [self._adj_handle(j, fused and j == J - 1) >= 0 for j in range(J)]}

    def _adj_handle(self, j: int, computes_readout: bool) -> int:
        """Kernel of adjoint pass j: the pass that computes the fused readout runs on the interpreter.  Compiled per
        plan, its cross entropy (expf / logf and fp32 sums of one thread per workgroup) gave dL/d<Z> different in the
        last bit for a share of the samples, and the paths must agree bitwise (with the readout kernel too:
        tests/test_gpu_hea.py).  Without the fused readout the same pass runs its per-plan kernel."""
        return -1 if computes_readout else self.spec_adj[j]

    def _count(self, handle: int) -> int:
        self.spec_launches += handle >= 0
        self.interp_launches += handle < 0
        return handle

    def spec_cfg(self, j: int, adjoint: bool) -> list:
        """Constants pass j's per-plan kernel is compiled with (hea_bindings.cpp spec_desc)."""
        p = self.passes[j].adj_pass if adjoint else self.passes[j].fwd_pass
        gen, load_lam, store_lam = (0, int(j < self.n_passes - 1), int(j > 0)) if adjoint else (int(self._gen(j)), 0, 0)
        glo = os.environ.get("QFEDX_EXTRA_HIPFLAGS", "")
        gate_lo = 0 if "-DQFX_HEA_GATE_LO=0" in glo else (1 if "-DQFX_HEA_GATE_LO=1" in glo else -1)
        from .. import _build
        return [self.n, p.t, p.c, p.lo, p.hi, self.C, gen, load_lam, store_lam,
                self.n_regions[j] if adjoint else 0] + [int(h) for h in p.H] + \
               [int(self.bf16), int(_build.variant() == "stamps"), gate_lo, int(self.obs_at_load)] + \
               ([int(self.spec_lean)] if self.spec_lean else [])     # (0: the list of before the knob)

    def prepare_spec(self) -> bool:
        """Compile (or load from ``QFEDX_JIT_CACHE``) the forward and adjoint kernel of every pass; on a failure warn
        once and stay on the interpreter."""
        global _SPEC_WARNED
        from .statevec_hip import ARCH, CSRC, JIT_CACHE
        JIT_CACHE = os.environ.get("QFEDX_JIT_CACHE", JIT_CACHE)     # (read per call: tests point it at a tmp dir)
        C = ext()
        fwd, adj, keys = [-1] * self.n_passes, [-1] * self.n_passes, []
        try:
            for j, ((f, ff), (a, fa)) in enumerate(self._host_progs):
                if (self.spec_gen or not self._gen(j)) and j <= self.fwd_last and len(f):
                    fwd[j], k = C.hea_spec_prepare(False, f, ff, self.spec_cfg(j, False), JIT_CACHE, CSRC, ARCH)
                    keys.append(k)
                if len(a):
                    adj[j], k = C.hea_spec_prepare(True, a, fa, self.spec_cfg(j, True), JIT_CACHE, CSRC, ARCH)
                    keys.append(k)
            if self.device.type == "cuda":
                with torch.cuda.device(self.device):     # (a module is loaded on the device it is launched on)
                    for h in fwd + adj:
                        if h >= 0:
                            C.hea_spec_load(h)
        except RuntimeError as e:
            if not _SPEC_WARNED:
                import warnings
                warnings.warn(f"per-plan MFMA pass kernels unavailable, using the interpreter: {e}")
                _SPEC_WARNED = True
            self.spec_fwd, self.spec_adj, self.spec_keys = [-1] * self.n_passes, [-1] * self.n_passes, []
            return False
        self.spec_fwd, self.spec_adj, self.spec_keys = fwd, adj, keys
        return True

    # ------------------------------------------------------------------ workspaces
    @contextlib.contextmanager
    def private_workspace(self, ws: dict):
        """Route workspace allocations to ``ws`` (owned by a captured hipGraph)."""
        saved = self._ws
        self._ws = ws
        try:
            yield ws
        finally:
            self._ws = saved

    def _zbuf(self, name: str, numel: int, dtype) -> torch.Tensor:
        """Workspace that is zero when created (e.g. arrival counters that their kernel resets after use): created
        outside graph capture (the capture's warm-up run), so no fill is ever captured."""
        t = self._ws.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.zeros(numel, dtype=dtype, device=self.device)
            self._ws[name] = t
        return t[:numel]

    def _buf(self, name: str, numel: int, dtype) -> torch.Tensor:
        t = self._ws.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.empty(numel, dtype=dtype, device=self.device)
            self._ws[name] = t
        return t[:numel]

    @property
    def n_passes(self) -> int:
        return len(self.passes)

    @property
    def tiles_last(self) -> int:
        """Tiles per sample of the pass that reads out <Z> (the last forward pass that runs)."""
        return 1 << (self.n - self.passes[self.fwd_last].fwd_pass.t)

    def _gen(self, j: int) -> bool:
        """Forward pass j generates the layer-1 product state in its tile (pass 0 of an angle program)."""
        return j == 0 and not self.amplitude

    def _geom(self, p, gen, load_lam, store_psi, store_lam, B, p_stride, S, x_stride, K, in_rep: int = 1,
              n_regions: int = 0, shared: bool = False):
        if self.amplitude:       # no pass reads feature angles (gen = 0 everywhere): the dummy column's stride is moot
            x_stride = max(int(x_stride), self.n)
        return [self.n, p.t, p.c, p.lo, p.hi, 1 << (self.n - p.t), int(gen), int(load_lam), int(store_psi),
                int(store_lam), B, self.C, self.n_theta, p_stride, self.feature, S, x_stride, self.n_slots,
                self.slab_tiles, K] + [int(h) for h in p.H] + [self.n_gradops, int(in_rep), int(self.bf16),
                                                                 int(n_regions), int(shared), int(self._nt_store(S))]

    def _nt_store(self, S: int) -> bool:
        """Non-temporal pass-output stores once a pass's states (S x 2^n x 4 bytes) outgrow half the 256 MB Infinity
        Cache: 16q x 2048 samples (512 MB) 1.820 -> 1.784 ms per step, while 8 clients' 64 MB are re-read faster from
        the cache with plain stores (profiles/r6_tile_nt_priority_ab.txt).  QFEDX_HEA_NT=0 / 1 overrides."""
        env = os.environ.get("QFEDX_HEA_NT")
        if env is not None:
            return env == "1"
        return S * (4 << self.n) > NT_STORE_MIN_BYTES

    def _frags(self, params: torch.Tensor, K: int, tag: str = "") -> torch.Tensor:
        fr = self._buf(f"{tag}frags", max(K * self.n_slots * 4 * 128 * 4, 1), torch.int32)
        if self.n_slots:
            ext().hea_frags(params, params.shape[1], self.slot_tab, self.n_slots, K, fr, self.bf16)
        return fr

    def _stage(self, init: torch.Tensor, K: int, B: int, tag: str = "") -> torch.Tensor:
        """Real ``init`` [K, B, F <= 2^n] raw amplitudes -> psi_in of forward pass 0 in a workspace buffer (owned by a
        captured round like every other): zero padded, normalised with a float64 norm (a zero row -> the uniform
        state), scaled and rounded once to the storage format on the device (csrc/hea_amp.hip)."""
        if init.dim() != 3 or init.shape[0] != K or init.shape[1] != B:
            raise ValueError(f"init must be [K, B, F] = [{K}, {B}, <= 2^{self.n}], got {tuple(init.shape)}")
        if init.shape[2] < 1 or init.shape[2] > (1 << self.n):
            raise ValueError(f"init has {init.shape[2]} amplitudes per sample, the state 2^{self.n}")
        x = init.reshape(K * B, init.shape[2])
        if x.dtype != torch.float32 or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
            x = x.float().contiguous()
        psi = self._buf(f"{tag}amp", (K * B) << self.n, torch.int32)
        ext().hea_amp_stage(x, self.n, psi, self.scale, self.bf16)
        return psi

    def _check_init(self, init) -> None:
        """Refuse an ``init`` this program cannot start from, saying why."""
        if not self.amplitude:
            if init is not None:
                raise ValueError("this MFMA program starts from the angle feature map: it takes no initial states "
                                 "(init is for feature_map='amplitude' specs)")
        elif init is None:
            raise ValueError("an amplitude-encoded MFMA program needs init [K, B, F <= 2^n] raw amplitudes")
        elif init.is_complex():
            raise ValueError("the MFMA engine encodes real amplitudes itself (normalised, real states); explicit "
                             "complex initial states run on the fp32 VALU engine (state_dtype=fp32)")

    def _start(self, init, K: int, B: int, tag: str = ""):
        """Staged input states of an amplitude program, None for an angle program."""
        self._check_init(init)
        return self._stage(init, K, B, tag) if self.amplitude else None

    def _launch(self, j: int, adjoint: bool, c: _Call, *, psi_in=None, psi_out=None, lam_in=None, lam_out=None,
                wread=None, part=None, gslab=None, readout=None, in_rep: int = 1) -> None:
        """Launch pass j, forward or adjoint: the only caller of ``hea_pass``.  The flags follow from the buffers given
        (store psi: ``psi_out``; load / store lambda: ``lam_in`` / ``lam_out``; a forward pass generates its input iff
        ``_gen(j)``, which must agree with an absent ``psi_in``); ``readout`` = [y, wts, expz, wread, rec]: an adjoint
        pass that computes the fused readout from ``part``, on the interpreter (``_adj_handle``)."""
        e = self.passes[j]
        p, tab = (e.adj_pass, e.adj) if adjoint else (e.fwd_pass, e.fwd)
        gen = not adjoint and self._gen(j)
        if not adjoint and gen != (psi_in is None or psi_in.numel() == 0):
            raise RuntimeError("forward pass without a start: amplitude programs need staged states")
        geom = self._geom(p, gen, lam_in is not None, psi_out is not None, lam_out is not None, c.B, c.params.shape[1],
                          c.K * c.B, c.x.shape[1], c.K, in_rep, self.n_regions[j] if adjoint else 0, c.shared)
        handle = self._adj_handle(j, readout is not None) if adjoint else self.spec_fwd[j]
        bufs = [self._iempty if t is None else t for t in (psi_in, psi_out, lam_in, lam_out)]
        outs = [self._fempty if t is None else t for t in (wread, part, gslab)]
        ext().hea_pass(adjoint, *tab, geom, self.scale, *bufs, c.x, c.params, c.fr, *outs,
                       c.dbg[f"{'adj' if adjoint else 'fwd'}{j}"] if c.dbg else _NODBG,
                       *(() if readout is None else (readout, self.tiles_last)), spec=self._count(handle))

    def _forward(self, x, params, fr, K, B, part, store_last: bool = False, tag: str = "", dbg=None,
                 shared: bool = False, psi0=None, first: int = 0, in_rep: int = 1, pingpong: str = "pe"):
        """Forward passes ``first``..``fwd_last`` (the readout pass); returns the stored pass outputs (all of them with
        ``store_last``: the adjoint starts each pass from its output; identity passes after ``fwd_last`` alias
        its output).  ``psi0``: the input of pass ``first`` (none: it generates), each row of it read by ``in_rep``
        consecutive samples.  ``tag`` names the workspaces, ``pingpong`` the two an evaluation alternates between;
        ``dbg`` (stamps build): per-pass stall-attribution buffers."""
        c = _Call(x, params, fr, K, B, shared, dbg)
        N = (K * B) << self.n
        stored, psi = [], psi0
        J, R = self.n_passes, self.fwd_last
        for j in range(first, R + 1):
            # evaluation only needs the previous pass output: two ping-pong buffers instead of one per pass
            name = f"{tag}psi{j}" if store_last else f"{tag}{pingpong}{(j - first) % 2}"
            out = self._buf(name, N, torch.int32) if j < R or store_last else None
            self._launch(j, False, c, psi_in=psi, psi_out=out, part=part if j == R else None,
                         in_rep=in_rep if j == first else 1)
            if out is not None:
                stored.append(out)
            psi = out
        if store_last:
            stored += [stored[R]] * (J - 1 - R)
        return stored

    def _adjoint(self, x, params, fr, K, B, stored, wread, gslab, tag: str = "", readout=None, dbg=None,
                 shared: bool = False):
        """Adjoint passes, last pass first.  ``readout`` = (part, y, wts, expz, rec): the first adjoint pass computes
        every sample's readout and dL/d<Z> itself (fused readout; ``wread`` is then its output, read by the later
        passes) instead of taking ``wread`` from the readout kernel."""
        c = _Call(x, params, fr, K, B, shared, dbg)
        lam_in = None
        for j in reversed(range(self.n_passes)):
            lam_out = self._buf(f"{tag}lam{j % 2}", (K * B) << self.n, torch.int32) if j > 0 else None
            ro = readout if j == self.n_passes - 1 else None
            self._launch(j, True, c, psi_in=stored[j], lam_in=lam_in, lam_out=lam_out, gslab=gslab,
                         wread=wread if ro is None else None, part=None if ro is None else ro[0],
                         readout=None if ro is None else [*ro[1:4], wread, ro[4]])
            lam_in = lam_out

    def _expect(self, x, th, K, B, z, tag: str = "", init=None, **fwd):
        """Fragments of ``th``, the forward passes (``_forward`` keywords) and <Z> summed into ``z`` [K B, C], in
        ``tag``'s workspaces -> (fragments, stored pass outputs).  ``init``: raw amplitudes to stage as the start."""
        fr = self._frags(th, K, tag)
        part = self._buf(f"{tag}part", K * B * self.tiles_last * self.C, torch.float32)
        if init is not None:
            fwd["psi0"] = self._stage(init, K, B, tag)
        stored = self._forward(x, th, fr, K, B, part, tag=tag, **fwd)
        ext().readout_sum(part, self.tiles_last, self.C, K * B, z)
        return fr, stored

    def _prep(self, xang, params):
        K, B, F = xang.shape
        if F < self.n and not self.amplitude:     # (an amplitude program reads no feature angles)
            raise ValueError(f"expected >= {self.n} feature angles per sample, got {F}")
        x = xang.reshape(K * B, F).float().contiguous()
        p = params.float().contiguous()
        if p.shape[0] != K:
            raise ValueError("one parameter row per client expected")
        return x, p, K, B

    def _pad_params(self, th: torch.Tensor) -> torch.Tensor:
        """Theta-only parameter rows zero-padded to the kernels' param stride (n_theta + the 2 C readout affines)."""
        short = self.n_theta + 2 * self.C - th.shape[1]
        return torch.cat([th, th.new_zeros(th.shape[0], short)], 1) if short > 0 else th

    def _need_prefix_reuse(self) -> None:
        """Prefix reuse starts shifted circuits from the chain forward's stored pass outputs and layer-1 product state."""
        if self.amplitude:
            raise ValueError("prefix-reuse parameter shift is angle-only: an amplitude program's shifted circuits run "
                             "as parameter rows of expz(init=...) (VQCEngine.param_shift_batched)")
        if self.ring:
            raise ValueError("prefix-reuse parameter shift is chain-only: a ring program's shifted circuits run as "
                             "parameter rows of expz (VQCEngine.param_shift_batched)")

    # ------------------------------------------------------------------ forward / eval
    @torch.no_grad()
    def expz(self, xang: torch.Tensor, theta: torch.Tensor, noise=None, keys=None, step: int = 0,
             init: torch.Tensor | None = None) -> torch.Tensor:
        x, th, K, B = self._prep(xang, theta)
        self._check_init(init)
        th = self._pad_params(th)
        S = K * B
        out = self._buf("expz", S * self.C, torch.float32)
        # clients per launch: two live states per sample fit the HBM budget (24q: 128 MiB per sample)
        Kc = max(1, min(K, self._shift_budget() // max(1, 2 * B * ((1 << self.n) * 4))))
        for k0 in range(0, K, Kc):
            k1 = min(K, k0 + Kc)
            self._expect(x[k0 * B:k1 * B], th[k0:k1] if Kc < K else th, k1 - k0, B, out[k0 * B * self.C:k1 * B * self.C],
                         init=init[k0:k1] if self.amplitude else None)     # (staged per client chunk)
        if noise is not None:
            from .statevec_hip import _keys
            ext().readout_noise(out, self.C, B, S, noise.p01, noise.p10, noise.shots, _keys(keys, noise), int(step))
        return out.reshape(K, B, self.C).clone()

    @torch.no_grad()
    def vjp(self, xang: torch.Tensor, theta: torch.Tensor, w: torch.Tensor, init: torch.Tensor | None = None):
        """Adjoint VJP of sum_c w[s, c] <Z_c>_s -> (<Z> [S, C], d/dtheta [K, n_theta])."""
        x, th, K, B = self._prep(xang, theta)
        psi0 = self._start(init, K, B)
        th = self._pad_params(th)
        S = K * B
        z = self._buf("expz", S * self.C, torch.float32)
        fr, stored = self._expect(x, th, K, B, z, store_last=True, psi0=psi0)
        wr = w.reshape(S, self.C).float().contiguous()
        gslab = self._buf("gslab", S * self.slab_tiles * self.n_gradops * 32, torch.int64)
        self._adjoint(x, th, fr, K, B, stored, wr, gslab)
        grad = torch.zeros(K, th.shape[1], dtype=torch.float32, device=self.device)
        ext().hea_grad_reduce(gslab, self.slab_tiles, self.n_gradops, self.gmeta, B, K, th, grad, th.shape[1])
        return z.view(S, self.C).clone(), grad[:, : self.n_theta]

    # ------------------------------------------------------------------ parameter shift (prefix reuse)
    def shift_owners(self) -> list:
        """Per forward pass j <= fwd_last: the theta indices whose rotation it applies (layer 1 is generated in
        pass 0; rotation group g of pass j carries theta_slot(layer, q) and its phase partner)."""
        self._need_prefix_reuse()
        own = [[] for _ in range(self.fwd_last + 1)]
        for q in range(self.n):
            own[0] += [self.plan.theta_slot(1, q), self.plan.theta_slot(1, q) + 1]
        for j in range(self.fwd_last + 1):
            for g in self.plan.passes[j].groups:
                for q in g.qubits:
                    own[j] += [self.plan.theta_slot(g.layer, q), self.plan.theta_slot(g.layer, q) + 1]
        flat = sorted(i for o in own for i in o)
        if flat != list(range(self.n_theta)):
            raise RuntimeError("forward passes do not own every parameter exactly once")
        return own

    def shift_pass_counts(self) -> dict:
        """Pass launches per sample of one parameter-shift gradient: naive (2 n_theta shifted circuits, every
        forward pass each) vs prefix reuse + the pi identity (one +pi branch per parameter from its pass on, the
        unshifted forward, C adjoint sweeps)."""
        F = self.fwd_last + 1
        own = self.shift_owners()
        branch = sum(len(o) * (F - j) for j, o in enumerate(own))
        return {"naive_fwd_passes": 2 * self.n_theta * F, "reuse_fwd_passes": branch + F,
                "reuse_adj_passes": self.C * self.n_passes, "branch_fwd_passes": branch}

    def _shift_budget(self) -> int:
        """Bytes of HBM the chunked evaluation / parameter-shift paths may hold in live states."""
        if self._ps_budget is None:
            env = os.environ.get("QFEDX_PS_BUDGET_MB")
            if env:
                self._ps_budget = int(env) << 20
            else:
                free, _ = torch.cuda.mem_get_info(self.device)
                self._ps_budget = int(0.4 * free)
        return self._ps_budget

    @torch.no_grad()
    def shifted_expz(self, xang: torch.Tensor, params: torch.Tensor, with_mean: bool = True) -> torch.Tensor:
        """Exact <Z> at theta +- pi/2 e_j for every client, parameter j, sign and sample -> [K, n_theta, 2, B, C]
        (sign 0: +pi/2), from the prefix-reuse identities of ``param_shift``.  ``with_mean=False`` drops the
        common term m (only the +- difference is wanted) and skips the +pi branches."""
        f0, fpi, jac = self._shift_parts(xang, params, with_mean)
        jt = jac.permute(0, 3, 1, 2)                        # [K, P, B, C]
        m = 0.5 * (f0.unsqueeze(1) + fpi) if with_mean else torch.zeros_like(jt)
        return torch.stack([m + jt, m - jt], 2).contiguous()

    @torch.no_grad()
    def _shift_parts(self, xang: torch.Tensor, params: torch.Tensor, with_mean: bool):
        """f(theta) [K, B, C], f(theta + pi e_j) [K, P, B, C] (None without the mean term) and the per-sample
        Jacobian d<Z_c>/dtheta_j [K, B, C, P]."""
        E = ext()
        x, th, K, B = self._prep(xang, params)
        P, C, n = self.n_theta, self.C, self.n
        th = self._pad_params(th)
        ps = th.shape[1]
        F = self.fwd_last + 1
        own = self.shift_owners()
        sb = (1 << n) * 4                                   # fp16 (re, im) per amplitude
        budget = self._shift_budget()
        Kc = max(1, min(K, (budget // 2) // max(1, (F + 3) * B * sb)))
        rows_max = max(B, (budget // 2) // (2 * sb))        # samples per +pi chunk (two ping-pong states)
        f0 = torch.empty(K, B, C, dtype=torch.float32, device=self.device)
        jac = torch.empty(K, B, C, P, dtype=torch.float32, device=self.device)
        fpi = torch.empty(K, P, B, C, dtype=torch.float32, device=self.device) if with_mean else None
        eye = torch.eye(C, dtype=torch.float32, device=self.device)
        for k0 in range(0, K, Kc):
            k1 = min(K, k0 + Kc)
            nk, S = k1 - k0, (k1 - k0) * B
            xs, ths = x[k0 * B:k1 * B], th[k0:k1].contiguous()
            z = self._buf("psz", S * C, torch.float32)
            fr, stored = self._expect(xs, ths, nk, B, z, "ps", store_last=True)
            f0[k0:k1] = z.view(nk, B, C)
            # per-sample Jacobian rows: one adjoint sweep per class over the stored forward, reduced with spc = 1
            gslab = self._buf("psgslab", S * self.slab_tiles * self.n_gradops * 32, torch.int64)
            th_rep = ths.repeat_interleave(B, 0).contiguous()
            g = torch.zeros(S, ps, dtype=torch.float32, device=self.device)
            for c in range(C):
                wr = eye[c].expand(S, C).contiguous()
                self._adjoint(xs, ths, fr, nk, B, stored, wr, gslab, "ps")
                E.hea_grad_reduce(gslab, self.slab_tiles, self.n_gradops, self.gmeta, 1, S, th_rep, g, ps)
                jac[k0:k1, :, c] = g[:, :P].view(nk, B, P)
            if not with_mean:
                continue
            # +pi branches: parameter rows (client, owned parameter) from their pass on
            per = max(1, rows_max // B)                     # parameter rows per chunk
            for j, sl in enumerate(own):
                if not sl:
                    continue
                Pj = len(sl)
                slots = torch.tensor(sl, dtype=torch.long, device=self.device)
                nr = min(Pj, per)
                nkc = max(1, per // Pj) if nr == Pj else 1
                for a0 in range(0, nk, nkc):
                    a1 = min(nk, a0 + nkc)
                    for r0 in range(0, Pj, nr):
                        r1 = min(Pj, r0 + nr)
                        src = stored[j - 1][(a0 * B) << n:(a1 * B) << n] if j > 0 else None
                        zb = self._pi_branch(j, xs[a0 * B:a1 * B], ths[a0:a1], slots[r0:r1], B, src)
                        fpi[k0 + a0:k0 + a1].index_copy_(1, slots[r0:r1], zb)
        return f0, fpi, jac

    @torch.no_grad()
    def param_shift(self, xang: torch.Tensor, params: torch.Tensor, w: torch.Tensor, noise=None, keys=None,
                    step: int = 0, exact_only: bool = False) -> torch.Tensor:
        """dL/dtheta by the parameter-shift rule with prefix reuse (ROADMAP.md:23,130-135).

        The naive estimator runs 2 n_theta shifted circuits per sample from |0>, each shot-sampled.  Two exact
        identities for a rotation exp(-i theta P / 2) (P^2 = 1) give the SAME shifted expectations with far
        fewer pass launches (``shift_pass_counts``):

          * f(theta +- pi/2) = m +- f'(theta),  m = (f(theta) + f(theta + pi)) / 2   (f = a + b cos + c sin)
          * f'(theta) for every parameter, sample and class = C adjoint sweeps (one per class, w = e_c) over the
            stored unshifted forward, reduced per sample (spc = 1)
          * f(theta + pi) for a parameter applied in forward pass j starts from the stored unshifted OUTPUT of
            pass j - 1 (the kernel's ``in_rep`` maps each shifted row to its client's stored sample) and runs
            only passes j..fwd_last; layer-1 parameters regenerate the product state in pass 0

        The exact shifted expectations are then readout-confused / shot-sampled exactly as the naive estimator
        samples them (same Philox key per (client, slot, sign) row: ``VQCEngine.param_shift_batched``), so the
        estimator's distribution is the hardware one.  With ``shots == 0`` the sampled difference is affine in
        f', so m is not needed (no +pi branches).  Work is chunked over clients and over shifted rows to fit
        ``_shift_budget`` (0.4 of free HBM).  ``exact_only``: skip the readout model (tests).
        w = dL/d<Z>_noisy [K, B, C] -> [K, n_theta]."""
        self._need_prefix_reuse()
        K, B, C = w.shape
        P = self.n_theta
        noisy = noise is not None and not exact_only
        need_m = noisy and noise.shots > 0
        f0, fpi, jac = self._shift_parts(xang, params, with_mean=need_m)
        # shifted expectations, their readout model and the shift rule in one device launch (HIP, qfx_ps_combine)
        out = torch.empty(K, P, dtype=torch.float32, device=self.device)
        kk = keys.to(self.device).long().contiguous() if (need_m and keys is not None) else _NO_KEYS.to(self.device)
        if need_m and keys is None:
            raise ValueError("shot sampling needs per-client Philox keys")
        fe = self._fempty
        ext().ps_combine(f0 if need_m else fe, fpi if need_m else fe, jac.contiguous(), w.float().contiguous(), kk,
                         noise.p01 if noisy else 0.0, noise.p10 if noisy else 0.0, noise.shots if noisy else 0,
                         int(step), int(noisy), out)
        return out

    def _pi_branch(self, j, xs, ths, slots, B, src) -> torch.Tensor:
        """<Z> of theta + pi e_slot for clients ths [na, ps] x slots [nr] owned by forward pass j: passes
        j..fwd_last, the first reading the clients' stored pass j - 1 outputs ``src`` [na B 2^n] (each row
        shared by nr parameter rows: in_rep) or, for j = 0, regenerating the product state.  -> [na, nr, B, C]"""
        na, nr = ths.shape[0], slots.numel()
        Kr, S = na * nr, na * nr * B
        ps = ths.shape[1]
        thr = ths.repeat_interleave(nr, 0).view(na, nr, ps).clone()
        thr[:, torch.arange(nr, device=self.device), slots] += float(np.pi)
        thr = thr.view(Kr, ps).contiguous()
        z = self._buf("pbz", S * self.C, torch.float32)
        self._expect(xs, thr, Kr, B, z, "pb", psi0=src, first=j, in_rep=nr, pingpong="psi")
        return z.view(na, nr, B, self.C)

    # ------------------------------------------------------------------ train step
    fuses_optimizer = True    # VQCEngine: loss_and_grads(fused_opt=...) may run the Adam step in the reduction

    def _fused_readout(self, noise) -> bool:
        """Noiseless steps compute the readout in the first adjoint pass (``fused_readout``)."""
        return noise is None and self.fused_readout and self.tiles_last * self.C <= 64

    def prologue_frag_job(self):
        """(slot_tab, frags) for the round prologue to build the first local step's fragments from the global
        parameters (one shared set: every client row starts as theta), or None without unitary slots.  The trainer
        then passes ``shared_frags=frags`` to that step's ``loss_and_grads`` (hea_frag.h; one launch fewer)."""
        if not self.n_slots:
            return None
        return [self.slot_tab, self._buf("pfrags", self.n_slots * 4 * 128 * 4, torch.int32)]

    def _head(self, x, p, K, B, shared_frags, dbg, psi0):
        """What a training step starts with: the fragments (the shared set or built from ``p``), the step's workspaces
        and the stored forward -> (adjoint(readout=None): runs the adjoint passes over it, part, wread, gslab)."""
        S = K * B
        shared = shared_frags is not None
        fr = shared_frags if shared else self._frags(p, K)
        part = self._buf("part", S * self.tiles_last * self.C, torch.float32)
        wread = self._buf("wread", S * self.C, torch.float32)
        gslab = self._buf("gslab", S * self.slab_tiles * self.n_gradops * 32, torch.int64)
        stored = self._forward(x, p, fr, K, B, part, store_last=True, dbg=dbg, shared=shared, psi0=psi0)

        def adjoint(readout=None):
            self._adjoint(x, p, fr, K, B, stored, wread, gslab, readout=readout, dbg=dbg, shared=shared)
        return adjoint, part, wread, gslab

    def _step(self, x, p, yy, ww, K, B, loss, correct, grad, expz, noise, keys, step, adam=None, dbg=None,
              shared_frags=None, fed=None, psi0=None):
        """Forward, readout + CE, adjoint and gradient reduction of clients [0, K).
        ``adam`` = (tensors, hyper) from ``BatchedOptimizer.fused_adam``: the clients' Adam step runs in the
        gradient reduction's epilogue (one launch fewer per local step).  ``dbg``: stall-attribution buffers per
        pass (``stamp_buffers``, stamps build only)."""
        C = ext()
        S = K * B
        adjoint, part, wread, gslab = self._head(x, p, K, B, shared_frags, dbg, psi0)
        # Fused readout: the first adjoint pass computes each sample's <Z>, cross entropy and dL/d<Z> from the readout
        # partials, and the gradient reduction sums the clients' loss, hits and readout gradients - one launch fewer
        # per local step.
        # Split readout (readout_mode): those per-sample values come from a launch of their own, once per sample instead of
        # once per adjoint tile, and the last adjoint pass - no longer the one that computes them - runs per plan.  The
        # records and the reduction are the fused route's, bit for bit.
        ro = None
        mode = self.readout_mode(S, noise)
        if mode == "kernel":
            model = (0.0, 0.0, 0, _NO_KEYS, 0)
            if noise is not None:
                from .statevec_hip import _keys
                model = (noise.p01, noise.p10, noise.shots, _keys(keys, noise), int(step))
            C.readout_ce(part, self.tiles_last, self.C, B, K, yy, ww, p, self.n_theta, expz, wread, loss, correct,
                         grad, True, *model)
            adjoint()
        else:
            rec = self._buf("rorec", S * (2 * self.C + 2), torch.float32)
            ro = [rec, loss, correct]
            if mode == "split":
                C.hea_readout_rec(part, self.tiles_last, self.C, B, K, yy, ww, p, self.n_theta, expz, wread, rec)
            adjoint(None if mode == "split" else (part, yy, ww, expz, rec))
        opt, tail = (None, None), ()
        if adam is not None:
            f = fed if fed is not None else {}
            opt = (adam[0] + [self._zbuf("adamcnt", K, torch.int32)], adam[1])
            tail = (f.get("fed"), bool(f.get("wrap", False)), int(f.get("n_norms", 0)))
        C.hea_grad_reduce(gslab, self.slab_tiles, self.n_gradops, self.gmeta, B, K, p, grad, p.shape[1], *opt, ro,
                          self.C, self.n_theta, *tail)

    def _dpsgd_step(self, x, p, yy, ww, K, B, loss, correct, grad, expz, noise, dpsgd, dbg=None, shared_frags=None,
                    psi0=None) -> dict:
        """One record-level DP-SGD step (csrc/hea_dpsgd.hip): the forward and adjoint passes of an ordinary step with
        0 / 1 sample weights - so a slab row is that sample's raw gradient - and the per-sample readout records of
        ``hea_readout_rec`` whatever the sample count; then ``hea_dp_norm`` (per-sample norm and clip factor) and
        ``hea_dp_reduce`` (clipped lot sum + sigma C z from the clients' device key table, over the nominal lot) in
        place of ``hea_grad_reduce``.  No circuit is evaluated twice.  ``ww``: a sample is live where its weight is
        positive.  Readout noise is refused: the readout / CE kernel route writes no per-sample record."""
        if noise is not None:
            raise ValueError("record-level DP-SGD on the MFMA engine needs a noiseless readout (noise.kind / readout "
                             "noise write no per-sample record)")
        if not self.grad_cover_exact or self.n_gradops == 0 or p.shape[1] != self.n_theta + 2 * self.C:
            raise ValueError("record-level DP-SGD needs every circuit parameter owned by exactly one gradient record "
                             "and parameter rows [n_theta + 2 C]")
        clip, sigma, lot = float(dpsgd["clip"]), float(dpsgd["sigma"]), float(dpsgd["lot"])
        if not (clip > 0 and sigma >= 0 and lot > 0):
            raise ValueError("dpsgd needs clip > 0, sigma >= 0 and lot > 0")
        kk = dpsgd.get("keys") if sigma > 0 else _NO_KEYS
        if sigma > 0:
            if kk is None or tuple(kk.shape) != (K, 2):
                raise ValueError("dpsgd noise needs the clients' Philox keys as a [K, 2] table")
            kk = kk.to(self.device).long().contiguous()      # (a device table already on the round path: no copy)
        C = ext()
        S = K * B
        live = (ww > 0).float()
        adjoint, part, wread, gslab = self._head(x, p, K, B, shared_frags, dbg, psi0)
        rec = self._buf("rorec", S * (2 * self.C + 2), torch.float32)
        norm = self._buf("dpnorm", S, torch.float64)
        cfac = self._buf("dpc", S, torch.float64)
        C.hea_readout_rec(part, self.tiles_last, self.C, B, K, yy, live, p, self.n_theta, expz, wread, rec)
        adjoint()
        C.hea_dp_norm(gslab, self.slab_tiles, self.n_gradops, self.gmeta, B, K, p, rec, self.C, self.n_theta, clip,
                      norm, cfac)
        C.hea_dp_reduce(gslab, self.slab_tiles, self.n_gradops, self.gmeta, B, K, p, rec, live, cfac, self.C,
                        self.n_theta, kk, int(dpsgd.get("step", 0)), sigma, clip, lot, grad, loss, correct)
        return {"loss": loss, "grad": grad, "correct": correct, "expz": expz.reshape(K, B, self.C),
                "dp_norm": norm.view(K, B), "dp_c": cfac.view(K, B)}

    def stamp_buffers(self) -> dict:
        """Zeroed stall-attribution buffers, one per pass launch (``fwd{j}``, ``adj{j}``), for the stamps build
        (``QFEDX_STAMPS=1``, scripts/hea_stamps.py)."""
        rows = int(getattr(ext(), "HEA_STAMP_ROWS", 0)) * 16
        names = [f"fwd{j}" for j in range(self.fwd_last + 1)] + [f"adj{j}" for j in range(self.n_passes)]
        return {nm: torch.zeros(rows, dtype=torch.int64, device=self.device) for nm in names}

    def loss_and_grads(self, xang, y, wmask, params, spec, noise=None, keys=None, step: int = 0, out_loss=None,
                       out_correct=None, init: torch.Tensor | None = None, fused_opt=None, dbg=None,
                       shared_frags=None, fed_tail=None, dpsgd=None) -> dict:
        """One adjoint training step (same contract as ``HipProgram.loss_and_grads``).
        ``fused_opt`` = (BatchedOptimizer, active): with params updated in place (a contiguous fp32 tensor) and HIP
        Adam, the optimizer step runs in the gradient reduction's epilogue and the result says ``opt_done``;
        otherwise the caller steps the optimizer itself.
        ``dpsgd`` = dict(clip, sigma, keys, step, lot): a record-level DP-SGD step (``_dpsgd_step``): ``grad`` is the
        clipped, noised lot gradient; never fused with the optimizer or the FedAvg tail (no ``opt_done``)."""
        x, p, K, B = self._prep(xang, params)
        psi0 = self._start(init, K, B)
        S = K * B
        yy = y.reshape(S).long().contiguous()
        ww = wmask.reshape(S).float().contiguous()
        expz = self._buf("expz", S * self.C, torch.float32)
        loss = torch.empty(K, dtype=torch.float32, device=self.device) if out_loss is None else out_loss
        correct = torch.empty(K, dtype=torch.float32, device=self.device) if out_correct is None else out_correct
        grad = torch.empty_like(p)
        if dpsgd is not None:
            return self._dpsgd_step(x, p, yy, ww, K, B, loss, correct, grad, expz, noise, dpsgd, dbg, shared_frags, psi0)
        adam = None
        # Fused only while the reduction has at most one block per CU.  Every block publishes its gradient entries
        # with one agent-scope release (an L2 writeback here): at 16q x 64 clients (832 blocks) the fused launch took
        # 33.6 us against 13 + 5.4 us for the two launches; at the 8-client share (104 blocks) it saves a launch
        # (round 387 -> 382 us; profiles/r3_fused_adam_ab.txt).
        ro_rows = 1 if self._fused_readout(noise) else 0
        # (the readout parameters are owned by the fused readout block, and the row must hold nothing else)
        want = (K * (self.n_gradops + ro_rows) <= FUSED_ADAM_MAX_BLOCKS and ro_rows == 1 and self.grad_cover_exact
                and p.shape[1] == self.n_theta + 2 * self.C)
        if want and fused_opt is not None and self.n_gradops > 0 and p.data_ptr() == params.data_ptr():
            adam = fused_opt[0].fused_adam(p, fused_opt[1])
        fed = fed_tail if (adam is not None and fed_tail is not None) else None
        self._step(x, p, yy, ww, K, B, loss, correct, grad, expz, noise, keys, step, adam=adam, dbg=dbg,
                   shared_frags=shared_frags, fed=fed, psi0=psi0)
        res = {"loss": loss, "grad": grad, "correct": correct, "expz": expz.reshape(K, B, self.C)}
        if adam is not None:
            res["opt_done"] = True
        if fed is not None:
            res["fed_done"] = True     # the round's FedAvg ran in the Adam epilogue (QfxFedTail)
        return res
