"""The device epilogue of a federated round on the HIP path (no server optimizer): the fused FedAvg reduce + metrics
pack (``reduce``), its fold into the MFMA engine's last local step (``fused_tail``), the round's one collective and
the in-place apply (``post``).  The trainer runs them behind the local steps, captured into the round's hipGraph."""
from __future__ import annotations

import os
from typing import Optional

import torch

from ..parallel.dist import all_reduce_
from .round_graph import RoundCtx

# single-rank rounds apply the update inside the FedAvg reduce launch (FusedApply: every block arrives on one counter)
# up to this many buffer entries: past it the arrivals, one same-address atomic per 64-parameter block, cost more
# than the round_apply launch they save (CFed TinyCNN, 128 clients: +9 us per round, profiles/r4_round_structure_ab.txt)
FUSED_APPLY_MAX = 4096


class DeviceRoundEpilogue:
    """Owns the epilogue's persistent device buffers, all allocated here, eagerly (created inside the round graph's
    capture, a buffer's zero fill would become a node replayed every round).  Round-dependent inputs travel as
    per-client tables with the round's upload, never as kernel arguments.  ``begin_round`` sets the round's host
    values (``r``, ``ids``, the global params); a replayed graph keeps what its capture saw of them."""

    def __init__(self, runner):
        p, dev = runner.cfg.privacy, runner.device
        self.p, self.agg, self.world, self.secagg = p, runner.aggregator, runner.world, runner.secagg
        self.client_dp = bool(getattr(runner, "client_dp", p.dp))
        self.uniform = runner.cfg.train.weighting == "uniform"
        self.noise_seed, self.num_clients = runner.noise_seed, runner.num_clients
        self.P, self.NN = runner.P, runner.n_norm_slots
        self.ring = (p.secagg_bits, p.secagg_scale) if p.secure_agg else (0, 1.0)
        # a single-rank round small enough applies inside the reduce launch (no collective in between)
        self.can_fold = not self.world.distributed and self.P + 6 + self.NN <= FUSED_APPLY_MAX
        self.buf = torch.zeros(self.P + 6 + self.NN, dtype=torch.int64, device=dev)     # the all-reduce buffer
        # [metrics | sat | wsum | norms], one per graph variant, and how often each was written (resolve_record)
        self.outs = [torch.zeros(6 + self.NN, dtype=torch.float64, device=dev) for _ in range(2)]
        self.out_writes = [0, 0]
        self.flip = 0                       # the variant the next eager post() takes
        self.apply_cnt = torch.zeros(1, dtype=torch.int32, device=dev)    # FusedApply arrivals (self-resetting)
        self.tail_cnt = torch.zeros(1, dtype=torch.int32, device=dev)     # fused-tail arrivals (self-resetting)
        self.mask_u8 = self.agg.angle_mask.to(torch.uint8).contiguous()
        self.applied: Optional[int] = None  # the variant whose apply the last reduce / fused tail folded in
        self.r, self.ids, self.params = 0, [], runner.params

    def begin_round(self, r: int, ids: list, params, participants: list, dropped: list, dp_scale) -> dict:
        """Set round r's host values and return its ``extra`` per-client tables."""
        self.r, self.ids, self.params = r, ids, params
        p, extra = self.p, {}
        if self.client_dp and ids:      # (record-level DP noises inside the local steps: the reduce adds nothing)
            from ..ops.fedavg_hip import dp_noise_keys
            extra["dpkeys"] = dp_noise_keys(ids, r, self.noise_seed)
        if self.uniform:
            extra["fw"] = torch.ones(len(ids), dtype=torch.float64)
        if dp_scale is not None and ids:
            extra["dpscale"] = torch.full((len(ids),), dp_scale, dtype=torch.float32)
        if p.secure_agg and ids:
            # SecAgg on the device: every local client's pair-seed keys and mask signs for this round ride with
            # the round's tables; the fused reduce masks each client's ring element (K18), so the round stays
            # one graph launch
            extra["sa_seed"], extra["sa_sign"] = self.secagg.round_tables(ids, participants, dropped,
                                                                          self.num_clients, r)
            extra["sa_round"] = torch.full((len(ids),), r, dtype=torch.int32)
        if self.NN and ids:
            extra["cid"] = torch.tensor(ids, dtype=torch.int32)
        return extra

    def _apply_variant(self, theta, ctx: RoundCtx) -> Optional[int]:
        """The metrics buffer variant whose post() the single-rank apply may fold into (None: no fold)."""
        # the variant captured right behind this call, or eagerly the one post() will take next
        v = ctx.variant if ctx.variant is not None else (self.flip if ctx.eager else None)
        return v if (v is not None and self.can_fold and theta.data_ptr() == self.params.data_ptr()) else None

    def fused_tail(self, tabs: dict, theta, ctx: RoundCtx) -> Optional[dict]:
        # plain FedAvg (no DP noise / clipping, no SecAgg masks) folded into the MFMA engine's fused Adam
        # epilogue of the last local step (hea_step.hip, QfxFedTail): same fixed-point terms, int64 atomics
        # into the zeroed buffer head, metrics packed and (single rank) the round applied by the last client
        if self.p.dp or self.p.secure_agg or self.NN or self.agg.backend != "hip" or \
                os.environ.get("QFEDX_FED_TAIL", "1") == "0":
            return None
        fed = [self.buf, theta, self.mask_u8, tabs.get("fw", tabs["w"]), tabs["loss"].reshape(-1),
               tabs["correct"].reshape(-1), tabs["nvalid"].reshape(-1), tabs["act"].reshape(-1), self.tail_cnt]
        v = self._apply_variant(theta, ctx)
        if v is not None:
            fed += [self.params, self.outs[v]]
        return {"fed": fed, "wrap": bool(self.agg.wrap), "n_norms": self.NN, "zero": self.buf[: self.P + 1]}

    def reduce(self, params_k, tabs: dict, theta, ctx: RoundCtx) -> None:
        # one launch: the fused reduce writes the buffer head, its last block packs the metrics.  Single rank,
        # with post(v) known to follow, the same launch also applies the round (no collective in between), one
        # launch fewer per round.  ctx.fed_done: the engine already ran all of it (fused_tail).
        v = self.applied = self._apply_variant(theta, ctx)
        if ctx.fed_done:
            return
        sa = (tabs["sa_seed"], tabs["sa_sign"], tabs["sa_round"]) if "sa_seed" in tabs else None
        apply = (self.params, self.outs[v], self.apply_cnt, *self.ring, self.NN) if v is not None else None
        buf = self.buf
        self.agg.local_reduce(params_k, theta, tabs.get("fw", tabs["w"]), self.r, self.ids, out=buf[: self.P + 1],
                              keys=tabs.get("dpkeys"), secagg_tabs=sa, norm_cid=tabs.get("cid"),
                              pack=(buf, tabs["loss"].reshape(-1), tabs["correct"].reshape(-1),
                                    tabs["nvalid"].reshape(-1), tabs["act"].reshape(-1)), apply=apply,
                              dp_scale=tabs.get("dpscale"))

    def post(self, v: int) -> None:
        # ONE collective per round (CC2+CC3), then finalize + apply in place; captured into the round graph
        # (variant v writes metrics buffer v) when the collective allows it.  A single-rank round whose reduce
        # already applied variant v (in the same capture, or eagerly just before) has nothing left to do.
        applied, self.applied = self.applied, None
        if applied == v:
            return
        all_reduce_(self.buf, self.world)
        from ..ops._ext import ext
        ext().round_apply(self.buf, self.P, self.params, 1.0, self.outs[v], *self.ring, self.NN)

    def take_variant(self) -> int:
        """The metrics buffer variant of a round whose post() the caller runs itself."""
        v = self.flip
        self.flip ^= 1
        return v
