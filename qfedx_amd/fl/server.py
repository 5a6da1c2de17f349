"""Federated round loop ("server.py", ROADMAP.md:34-39; reference ``federated_learning``,
``Classical_FL.py:104-157``).

Reference behaviour kept: round-0 evaluation, ``num_rounds`` rounds of (all clients train ->
FedAvg -> load -> test eval), an accuracy history list, progress print every 5 rounds, return
``{'model', 'accuracies'}``.  Redesigned for MI355X:

* every rank holds an identical global parameter vector; clients are sharded over ranks and a
  rank's participating clients train as ONE batch (no per-client Python loop);
* client sampling (fraction q) and dropouts are keyed by (seed, round) so all ranks agree without
  communication; dropped clients simply contribute weight 0 (SecAgg orphan masks are removed);
* aggregation = fused local reduce on-device + ONE all-reduce of [update | weight | metrics];
* the test set is sharded over ranks and metrics are all-reduced;
* RDP accountant step + epsilon per round, JSONL metrics, checkpoint every K rounds, resume.
"""
from __future__ import annotations

import json
import math
import os
import time
from typing import Optional

import numpy as np
import torch

from ..parallel.dist import (ShardedServerState, World, agree_graph_comm, all_gather_cat, all_reduce_,
                             all_reduce_async, barrier, broadcast_, shard_clients)
from ..privacy.accountant import RDPAccountant
from ..privacy.dp import noise_scale, draw_noise_seed
from ..privacy.secure_agg import SecureAggregator
from ..utils.device import h2d
from ..utils.checkpoint import latest_checkpoint, load_checkpoint, save_checkpoint
from ..utils.logging import MetricsWriter, get_logger
from ..utils.seeding import generator, np_rng
from ..utils.timing import PhaseTimer
from .aggregator import EXACT_SCALE, Aggregator
from .epilogue import DeviceRoundEpilogue
from .trainer import ShardStore


def cc4_modes(runtime, distributed: bool) -> tuple:
    """CC4, ``(host_prefetch, device_side_stream)``: round r + 1's theta-independent work overlaps round r's
    collective - on the host (async all-reduce + ``_prefetch``), and on the graphed HIP round's side stream (opt-in:
    see ``RuntimeConfig.overlap_comm_device``).  With more than one rank; QFEDX_CC4=0 / 1 overrides both."""
    env = os.environ.get("QFEDX_CC4")
    if env is not None:
        return env == "1", env == "1"
    return distributed and bool(runtime.overlap_comm), distributed and bool(runtime.overlap_comm_device)


def sample_participants(num_clients: int, fraction: float, seed: int, round_num: int,
                        poisson: bool = False) -> list[int]:
    """Clients taking part in round ``round_num`` (ROADMAP.md:35,106), keyed by (seed, round) so every
    rank draws the same set without communication.

    ``poisson=False``: a fixed-size subset of m = round(q N) drawn without replacement.
    ``poisson=True``: every client independently with probability q (the set may be empty) - the
    sampling the subsampled-Gaussian RDP bound of ``privacy/accountant.py`` assumes."""
    if fraction >= 1.0:
        return list(range(num_clients))
    if poisson:
        u = np_rng(seed, "sample_clients_poisson", round_num).random(num_clients)
        return [int(c) for c in np.flatnonzero(u < fraction)]
    m = max(1, int(round(fraction * num_clients)))
    g = generator(seed, "sample_clients", round_num)
    return sorted(torch.randperm(num_clients, generator=g)[:m].tolist())


def sample_dropouts(participants: list[int], prob: float, seed: int, round_num: int) -> list[int]:
    if prob <= 0:
        return []
    out = []
    for c in participants:
        if np_rng(seed, "client_drop", round_num, c).random() < prob:
            out.append(c)
    return out


class FederatedRunner:
    """Drives federated training for one model adapter (VQC or TinyCNN) on this rank."""

    def __init__(self, cfg, adapter, data, world: World, device: torch.device, backend: str):
        self.cfg = cfg
        self.adapter = adapter
        self.data = data
        self.world = world
        self.device = device
        self.backend = backend
        self.log = get_logger()
        t, p = cfg.train, cfg.privacy
        self.num_clients = data.num_clients
        self.local_ids = list(data.client_ids)
        self.store = ShardStore(data.clients, data.client_ids, device)
        self.P = adapter.n_params
        # DP noise + DP client sampling key: a per-run secret (rank 0's OS randomness, broadcast, never
        # persisted or logged); the public train.seed only under privacy.deterministic_noise
        self.noise_seed = draw_noise_seed(world, p.deterministic_noise, t.seed) if p.dp else t.seed
        sampling = t.sampling if t.sampling != "auto" else ("poisson" if p.dp else "fixed")
        if sampling not in ("fixed", "poisson"):
            raise ValueError(f"train.sampling must be auto | fixed | poisson, got {t.sampling!r}")
        self.poisson = sampling == "poisson"
        noise_scale(getattr(p, "noise_mode", "local"), 1)           # validates privacy.noise_mode
        level = getattr(p, "level", "client")
        if level not in ("client", "record"):
            raise ValueError(f"privacy.level must be client | record, got {level!r}")
        # record-level DP (DP-SGD inside the local steps): the aggregator then neither clips nor noises
        self.record_dp = bool(p.dp) and level == "record"
        self.client_dp = bool(p.dp) and not self.record_dp
        if str(t.optimizer).lower() == "qng":
            self._setup_qng()
        if self.record_dp:
            self._setup_record_dp()
        if p.dp and getattr(p, "noise_mode", "local") == "distributed" and not p.secure_agg:
            # each client's share of the noise is too small to protect its update on its own: only the SecAgg sum
            # (which the server sees instead of the shares) carries the accounted sigma C
            raise ValueError("privacy.noise_mode=distributed needs privacy.secure_agg=true")
        if p.dp and getattr(p, "noise_mode", "local") == "distributed" and t.weighting != "uniform":
            # the shares are scaled by each client's FedAvg weight AFTER noising: the sum then carries noise std
            # sigma C sqrt(sum w_k^2 / m) against a sensitivity of max_k w_k C, an effective multiplier of
            # sigma RMS(w) / max(w) < sigma for unequal weights - the accountant would under-report epsilon
            raise ValueError("privacy.noise_mode=distributed needs train.weighting=uniform (with sample weighting "
                             "the aggregate noise falls below the accounted sigma)")
        self.secagg = None
        if p.secure_agg:
            # each client's DH secret comes from OS randomness on the rank hosting it; only public keys
            # are exchanged (all-gather), so no process holds another rank's client secrets
            self.secagg = SecureAggregator(None, p.secagg_bits, p.secagg_scale, getattr(p, "secagg_graph", "full"),
                                           getattr(p, "secagg_min_live", 0))
            self.secagg.setup(self.local_ids, world)
        self.aggregator = Aggregator(self.P, adapter.angle_mask(), device, backend, t.aggregate,
                                     t.wrap_angles, self.client_dp, p.clip_norm, p.noise_multiplier, p.secure_agg,
                                     self.secagg, self.noise_seed, num_clients=self.num_clients)
        self.accountant = RDPAccountant()
        # test shard for this rank
        Xt, yt = data.test
        sl = shard_clients(int(yt.shape[0]), world.world_size, world.rank)
        self.X_test = Xt[sl[0]: sl[-1] + 1].to(device) if sl else Xt[:0].to(device)
        self.y_test = yt[sl[0]: sl[-1] + 1].to(device) if sl else yt[:0].to(device)
        self.metrics = MetricsWriter(cfg.runtime.metrics_path, world.rank, cfg.to_dict(), cfg.runtime.tracking_dir,
                                     cfg.runtime.experiment or cfg.name)
        self.timer = PhaseTimer(device, every=int(cfg.runtime.timer_every or
                                                  (16 if torch.device(device).type == "cuda" else 1)))
        self.start_round = 0
        self.history: list[dict] = []
        self.server_opt = None
        if t.server_optimizer != "fedavg" or t.server_lr != 1.0:
            if p.secure_agg:
                raise ValueError("server_optimizer needs plain (non-SecAgg) aggregation of the update sums")
            self.server_opt = ShardedServerState(self.P, world, device, t.server_optimizer, t.server_lr,
                                                 t.server_momentum)
        self.params = adapter.init_params(t.seed).to(device)
        broadcast_(self.params, world)                      # CC1: identical theta on all ranks
        # CC6: per-client update norms in the round all-reduce.  Opt-in NON-PRIVATE diagnostic: the raw pre-clip norms
        # (and the clip fraction / quantiles logged from them) are computed from private data without noise and are
        # not charged to the accountant, so a run that logs them is outside the epsilon it reports
        self.n_norm_slots = self.num_clients if (self.client_dp and not p.secure_agg
                                                 and cfg.runtime.log_client_norms) else 0
        # CC2: the round's collective captured into the round hipGraph - decided ONCE, agreed by every rank (each
        # rank captures and replays one all-reduce, compared bitwise with an eager one; fl/trainer.py keeps a per-shape
        # eager fallback that preserves the collective order)
        want = (bool(cfg.runtime.graph_comm) and backend == "hip" and self.server_opt is None
                and torch.device(device).type == "cuda" and (not world.distributed or world.backend == "nccl"))
        self.graph_comm = agree_graph_comm(world, want)
        self.cc4, adapter.trainer.cc4 = cc4_modes(cfg.runtime, world.distributed)
        self.graph_comm_mode = ("captured" if self.graph_comm else "eager") if backend == "hip" else "none"
        # CC4 prefetch of the next round (round, setup, RoundPrefetch), and how many were built
        self._pre = None
        self.prefetches = 0
        self._counts_dev = self.store.counts.to(torch.float64).to(device)
        # the device round epilogue (HIP, no server optimizer): FedAvg reduce, collective and apply on the device
        self.epilogue = DeviceRoundEpilogue(self) if backend == "hip" and self.server_opt is None else None

    # ------------------------------------------------------------------ quantum natural gradient
    def _setup_qng(self) -> None:
        """``train.optimizer: qng``: refuse what the Fubini-Study metric does not cover, naming the config key.  Client
        level DP and SecAgg stay available: they act on the whole update."""
        cfg, t = self.cfg, self.cfg.train
        what = "train.optimizer=qng"
        if cfg.model.kind != "vqc":
            raise ValueError(f"{what} preconditions circuit angles: model.kind=vqc only, got {cfg.model.kind!r}")
        if not float(getattr(t, "qng_damping", 1e-3)) > 0:
            raise ValueError(f"train.qng_damping must be > 0 (a block is singular whenever its reference state is an "
                             f"eigenstate of a generator), got {t.qng_damping}")
        if cfg.noise.kind != "none":
            raise ValueError(f"{what} needs noise.kind=none, got {cfg.noise.kind!r}: the metric is a pure-state quantity")
        if self.record_dp:
            raise ValueError(f"{what} does not combine with privacy.level=record: the metric is computed from the lot's "
                             "records without clipping or noise, so the step would not be DP (privacy.level=client "
                             "and privacy.secure_agg act on the whole update and stay available)")
        from ..ops.qng import refusal
        why = refusal(self.adapter.spec, getattr(self.adapter, "noise", None),
                      getattr(self.adapter, "simulator", "statevector"))
        if why:
            raise ValueError(why)
        eng, need = self.adapter.engine, 2 * 8 * (1 << int(cfg.model.n_qubits))
        if eng.state_budget_bytes() < need:
            raise ValueError(f"{what} needs two states of one sample in the state budget: model.n_qubits="
                             f"{cfg.model.n_qubits} needs {need} bytes, the budget is {eng.state_budget_bytes()}")

    # ------------------------------------------------------------------ record-level DP
    def _setup_record_dp(self) -> None:
        """``privacy.dp`` with ``privacy.level: record``: refuse what the mechanism does not cover (naming the config
        key), agree on the sampling rate and the lot width, and hand the trainer its DP-SGD settings."""
        import torch.distributed as tdist
        cfg, t, p = self.cfg, self.cfg.train, self.cfg.privacy
        what = "privacy.level=record"
        if getattr(p, "noise_mode", "local") == "distributed":
            raise ValueError(f"{what} adds its noise inside every local step: privacy.noise_mode=distributed (shares "
                             "of a client-level noise) does not apply, use privacy.noise_mode=local")
        if cfg.model.kind != "vqc":
            raise ValueError(f"{what} needs per-sample gradients: model.kind=vqc only, got {cfg.model.kind!r}")
        method = "spsa" if t.optimizer == "spsa" else t.grad_method
        if method != "adjoint" and not (method == "autograd" and self.backend == "torch"):
            raise ValueError(f"{what} needs train.grad_method=adjoint (autograd on the torch backend), got {method!r}: "
                             "param_shift and spsa form no per-sample gradients")
        if getattr(self.adapter, "noise", None) is not None:
            raise ValueError(f"{what} needs a noiseless simulator: noise.kind={cfg.noise.kind!r} (gate / readout "
                             "noise, shots) is not covered")
        if getattr(self.adapter, "simulator", "statevector") != "statevector":
            raise ValueError(f"{what} runs on model.simulator=statevector, got {self.adapter.simulator!r}")
        eng = self.adapter.engine
        if eng.backend == "hip" and not hasattr(eng.hip, "_dpsgd_step"):
            raise ValueError(f"{what} on the HIP backend runs on the MFMA statevector engine: set model.state_dtype="
                             "mfma | fp16 | mfma_bf16 for a circuit it covers (>= 8 qubits), or runtime.backend=torch")
        if not (p.clip_norm > 0 and p.noise_multiplier >= 0):
            raise ValueError(f"{what} needs privacy.clip_norm > 0 and privacy.noise_multiplier >= 0")
        # q_max = max_k min(1, B / n_k) and the largest shard (the lot tables' width), identical on every rank: shard
        # sizes are only known where the shards live, so ONE MAX all-reduce of (n_max, -n_min)
        n = self.store.counts[self.store.counts > 0].double()
        ext = torch.tensor([float(n.max()) if n.numel() else 0.0, -float(n.min()) if n.numel() else -float("inf")],
                           dtype=torch.float64, device=self.world.device)
        if self.world.distributed:
            all_reduce_(ext, self.world, op=tdist.ReduceOp.MAX)
        n_max, n_min = int(ext[0].item()), -float(ext[1].item())
        if n_max <= 0:
            raise ValueError(f"{what}: no client holds a record")
        self.dp_q_max = min(1.0, t.batch_size / n_min)
        # local steps charged per round: the most any client can run (local_steps, or local_epochs x ceil(n_max / B))
        self.dp_round_steps = int(t.local_steps) if t.local_steps > 0 else \
            int(t.local_epochs) * int(math.ceil(n_max / t.batch_size))
        self.adapter.trainer.dpsgd = {"clip": float(p.clip_norm), "sigma": float(p.noise_multiplier),
                                      "seed": self.noise_seed, "nmax": n_max}

    def _dpsgd_tables(self, r: int, ids: list) -> dict:
        """Round r's per-client DP-SGD noise keys ``philox_key(noise_seed, 'dpsgd_noise', r, client)`` as an ``extra``
        table [K, 2]: they travel with the round's upload and reach the engine from the device table."""
        if not (self.record_dp and ids):
            return {}
        from ..utils.seeding import philox_keys
        return {"dpsgd_keys": torch.tensor(philox_keys(self.noise_seed, ("dpsgd_noise", r), ids), dtype=torch.int64)}

    # ------------------------------------------------------------------ eval
    @torch.no_grad()
    def evaluate(self, params: Optional[torch.Tensor] = None) -> dict:
        params = self.params if params is None else params
        loss_sum, correct, n = self.adapter.evaluate(params, self.X_test, self.y_test)
        buf = torch.tensor([loss_sum, correct, n], dtype=torch.float64, device=self.device)
        all_reduce_(buf, self.world)
        n_tot = max(float(buf[2]), 1.0)
        return {"test_acc": float(buf[1]) / n_tot, "test_loss": float(buf[0]) / n_tot}

    @torch.no_grad()
    def test_auc(self, params: Optional[torch.Tensor] = None) -> float:
        """Macro one-vs-rest ROC AUC on the full (rank-sharded, gathered) test set (ROADMAP:112)."""
        if not hasattr(self.adapter, "logits"):
            return float("nan")
        params = self.params if params is None else params
        lg = self.adapter.logits(params, self.X_test).float()
        C = self.cfg.model.n_classes
        probs = all_gather_cat(torch.softmax(lg, -1).reshape(-1), self.world).reshape(-1, C).cpu().numpy()
        ys = all_gather_cat(self.y_test.to(lg.device).double(), self.world).cpu().numpy().astype(int)
        try:
            from sklearn.metrics import roc_auc_score
            if C == 2:
                return float(roc_auc_score(ys, probs[:, 1]))
            if len(set(ys.tolist())) < C:
                return float("nan")
            return float(roc_auc_score(ys, probs, multi_class="ovr", average="macro"))
        except Exception:
            return float("nan")

    # ------------------------------------------------------------------ checkpoint
    def save(self, round_num: int) -> None:
        rt = self.cfg.runtime
        if not rt.checkpoint_dir:
            return
        # the sharded server-optimizer moments are gathered on every rank (collective) before rank 0 writes
        server_state = self.server_opt.state_dict() if self.server_opt is not None else None
        if self.world.is_main:
            payload = {
                "global_state": self.adapter.state_dict(self.params),
                "accountant": json.dumps(self.accountant.state_dict()),
                "config": self.cfg.to_dict(),
                "metrics": self.history,
                "seed": torch.tensor(self.cfg.train.seed),   # public root seed (DP noise uses a run secret)
            }
            if server_state is not None:
                payload["server_state"] = server_state
            path = save_checkpoint(rt.checkpoint_dir, round_num, payload)
            self.metrics.tracker.log_artifact(path, "checkpoints")
        barrier(self.world)

    def maybe_resume(self) -> None:
        rt = self.cfg.runtime
        if not (rt.resume and rt.checkpoint_dir):
            return
        path = latest_checkpoint(rt.checkpoint_dir)
        if path is None:
            return
        ck = load_checkpoint(path)
        self.params = self.adapter.from_state_dict(ck["global_state"]).to(self.device)
        self.accountant.load_state_dict(json.loads(ck["accountant"]))
        self.history = list(ck.get("metrics", []))
        if self.server_opt is not None:
            if "server_state" not in ck:
                raise ValueError(f"{path} has no server_state but train.server_optimizer="
                                 f"{self.cfg.train.server_optimizer!r} needs its moments to resume")
            self.server_opt.load_state_dict(ck["server_state"])
        self.start_round = int(ck["round"])
        self.log.info(f"resumed from {path} at round {self.start_round}")

    # ------------------------------------------------------------------ main loop
    def _round_setup(self, r: int) -> dict:
        """Round r's public, theta-independent decisions: participants, dropouts, the SecAgg abort, this rank's live
        clients.  Keyed by (seed, round) only, so computing them a round early (CC4 prefetch) changes nothing."""
        t = self.cfg.train
        p = self.cfg.privacy
        # under DP the participant set is part of the mechanism: keyed by the secret like the noise
        participants = sample_participants(self.num_clients, t.client_fraction,
                                           self.noise_seed if p.dp else t.seed, r, self.poisson)
        dropped = sample_dropouts(participants, t.dropout_prob, t.seed, r)
        # SecAgg+ abort (Bell et al.): a survivor left with fewer than the threshold of live mask neighbours would be
        # unmasked by the orphan-mask removal, so the round aggregates nothing.  The decision uses public data only
        # (participants, dropouts, the round-keyed graph): every rank takes it alike and still posts its (zero)
        # contribution to the one collective.
        sa_abort = bool(p.secure_agg and self.secagg is not None and participants
                        and not self.secagg.round_ok(participants, dropped, r))
        if sa_abort:
            dropped = list(participants)
        dropped_set = set(dropped)
        part_set = set(participants)
        local_part = [i for i, c in enumerate(self.local_ids) if c in part_set]
        local_alive = [i for i in local_part if self.local_ids[i] not in dropped_set]
        return {"participants": participants, "dropped": dropped, "sa_abort": sa_abort, "dropped_set": dropped_set,
                "local_alive": local_alive}

    def _prefetch(self, r: int) -> None:
        """CC4: build round r's theta-independent inputs now - its setup and, through the trainer, the minibatch plan,
        the tables and the gathered, encoded minibatches - while the previous round's collective is in flight."""
        if r >= self.cfg.train.num_rounds or not hasattr(self.adapter.trainer, "prepare_round"):
            return
        st = self._round_setup(r)
        dpx = self._dpsgd_tables(r, [self.local_ids[i] for i in st["local_alive"]])
        pre = self.adapter.trainer.prepare_round(self.store, st["local_alive"], r, **({"extra": dpx} if dpx else {}))
        self._pre = (r, st, pre)
        self.prefetches += 1

    def run_round(self, r: int, sync: bool = True) -> dict:
        """One federated round.  With ``sync=False`` nothing reads device memory back: the round is
        only enqueued (the host can build round r+1 while the GPU runs round r) and the returned
        record holds device tensors until :meth:`resolve_record`."""
        t = self.cfg.train
        p = self.cfg.privacy
        self.timer.step(r)
        pre_r, self._pre = self._pre, None
        pre = None
        if pre_r is not None and pre_r[0] == r:
            st, pre = pre_r[1], pre_r[2]
        else:
            st = self._round_setup(r)
        participants, dropped, sa_abort = st["participants"], st["dropped"], st["sa_abort"]
        dropped_set, local_alive = st["dropped_set"], st["local_alive"]
        t0 = time.perf_counter()
        dev = self.device
        P = self.P
        ids = [self.local_ids[i] for i in local_alive]
        # distributed DP: each client's share of the noise is N(0, sigma^2 C^2 / m) for the round's m live participants
        # (public: every rank knows the participant set and the dropouts), so the SecAgg sum carries exactly sigma C
        dp_mode = getattr(p, "noise_mode", "local")
        dp_scale = noise_scale(dp_mode, len(participants) - len(dropped)) if (self.client_dp and dp_mode != "local") \
            else None
        epi = self.epilogue
        fast = epi is not None
        trainer = self.adapter.trainer
        if fast:
            # the round epilogue on the device (fl/epilogue.py), run by the trainer right after the local steps and
            # captured with them into the round's hipGraph; post (collective + apply) too when the ranks agreed on it
            extra = {**epi.begin_round(r, ids, self.params, participants, dropped, dp_scale),
                     **self._dpsgd_tables(r, ids)}
            with self.timer.phase("local_train"):
                res = trainer.run_round(self.store, local_alive, self.params, r, epilogue=epi, extra=extra or None,
                                        post=epi.post if self.graph_comm else None)
            if not local_alive:
                epi.buf.zero_()
        else:
            with self.timer.phase("local_train"):
                res = trainer.run_round(self.store, local_alive, self.params, r,
                                        **({"pre": pre} if pre is not None else {}),
                                        **({"extra": self._dpsgd_tables(r, ids)} if self.record_dp else {}))
            with self.timer.phase("aggregate"):
                if t.weighting == "uniform":
                    w = torch.ones(len(local_alive), dtype=torch.float64, device=dev)
                elif "weights" in res:            # uploaded with the round's tables (no gather launch)
                    w = res["weights"]
                else:
                    w = self._counts_dev[res["lid"]]
                if local_alive:
                    contrib = self.aggregator.local_reduce(res["params"], self.params, w, r, ids,
                                                           participants=participants, dropped=dropped,
                                                           dp_scale=dp_scale)
                else:
                    contrib = torch.zeros(P + 1, dtype=torch.int64, device=dev)
                loss_sum = (res["loss"].double() * res["nvalid"].double()).sum()
                correct = (res["correct"].double() * res["act"].double()).sum()
                host_m = h2d(torch.tensor([float(res.get("samples", 0.0)), float(res.get("steps", 0))],
                                          dtype=torch.float64), dev)
                sat = self.aggregator.last_saturation if local_alive else None
                sat = (sat.to(dev).double().reshape(1) if sat is not None
                       else torch.zeros(1, dtype=torch.float64, device=dev))
                # CC6: this rank's clients' norms in their global slots (zero elsewhere): the metric SUM all-reduce
                # gathers them
                nslots = torch.zeros(self.n_norm_slots, dtype=torch.float64, device=dev)
                if self.n_norm_slots and local_alive and self.aggregator.last_norms is not None:
                    nslots[torch.tensor(ids, device=dev)] = self.aggregator.last_norms.double().to(dev)
                metrics = torch.cat([torch.stack([loss_sum, correct]).to(dev), host_m, sat, nslots])
        norms = None
        comm_bytes = 0
        with self.timer.phase("comm"):
            if fast:
                if res.get("post_done"):
                    v = res["post_variant"]
                else:
                    v = epi.take_variant()
                    epi.post(v)
                epi.out_writes[v] += 1
                comm_bytes = epi.buf.numel() * 8
                out = epi.outs[v]
                metrics = out[:5]                                     # + saturated fixed-point terms
                norms = out[6:6 + epi.NN] if epi.NN else None
            elif self.server_opt is not None:
                # server optimizer (CC5): small all-reduce of [weight | metrics]; the update sums are
                # reduce-scattered inside the sharded step and the new params all-gathered
                tail = torch.cat([contrib[P:P + 1].to(torch.int64),
                                  torch.round(metrics.double() * EXACT_SCALE).to(torch.int64)])
                all_reduce_(tail, self.world)
                # + the reduce-scatter of the padded update sums and the all-gather of the new parameter slices
                comm_bytes = tail.numel() * 8 + 2 * self.server_opt.padded * 8
                wsum = tail[0].double() / EXACT_SCALE
                metrics = tail[1:].double() / EXACT_SCALE
                self._set_params(self.server_opt.step(self.params, contrib[:P].to(torch.int64), wsum))
            elif p.secure_agg:
                all_reduce_(contrib, self.world)          # int64 ring elements: exact, mod later
                all_reduce_(metrics, self.world)
                comm_bytes = contrib.numel() * contrib.element_size() + metrics.numel() * metrics.element_size()
                mean_upd, wsum = self.aggregator.finalize(contrib)
                self._set_params(self.aggregator.apply(self.params, mean_upd, wsum=wsum))
            else:
                # ONE collective per round (CC2+CC3): [exact fixed-point update | weight | metrics]
                buf = torch.cat([contrib.to(torch.int64),
                                 torch.round(metrics.double() * EXACT_SCALE).to(torch.int64)])
                if self.cc4:
                    # CC4: round r + 1's theta-independent work (setup, plan, minibatch gather + encode) runs while
                    # this round's all-reduce is in flight (gloo: on its worker thread); theta_{r+1} waits for it
                    work = all_reduce_async(buf, self.world)
                    self._prefetch(r + 1)
                    work.wait()
                else:
                    all_reduce_(buf, self.world)
                comm_bytes = buf.numel() * 8
                mean_upd, wsum = self.aggregator.finalize(buf[: P + 1])
                metrics = buf[P + 1:].double() / EXACT_SCALE
                self._set_params(self.aggregator.apply(self.params, mean_upd, wsum=wsum))
        if not fast and self.n_norm_slots:
            norms, metrics = metrics[5:], metrics[:5]
        if self.record_dp:
            # record-level DP-SGD: every local step of a client is one subsampled-Gaussian step on its records at
            # rate q_k <= q_max; a record sits in one client's shard, so the round costs that client's steps, charged
            # at the most any client runs.  Conservative: the amplification by client sampling (a record's client
            # takes part in a round with probability client_fraction only) is ignored.
            self.accountant.step(self.dp_q_max, p.noise_multiplier, self.dp_round_steps)
        elif p.dp:
            # the subsampled-Gaussian RDP bound holds for Poisson sampling at rate q; a fixed-size subset
            # drawn without replacement is accounted conservatively with no amplification (q = 1)
            q = min(1.0, t.client_fraction) if self.poisson else 1.0
            self.accountant.step(q, p.noise_multiplier, 1)
        rec = {"round": r + 1, "participants": len(participants), "dropped": len(dropped), "secagg_aborted": sa_abort,
               "_metrics": metrics, "_t0": t0,
               "_out_stamp": (v, self.epilogue.out_writes[v]) if fast else None,
               "_norms": (norms, [c for c in participants if c not in dropped_set]) if norms is not None else None,
               "comm_bytes_per_rank": int(comm_bytes),
               "upload_bytes": int(len(participants) - len(dropped)) * (self.P + 1) * 4}
        if p.dp:
            rec["epsilon"] = self.accountant.get_epsilon(p.delta)      # per client, or per record (dp_level)
        if self.record_dp:
            rec["dp_level"] = "record"
            # records dropped from over-full Poisson lots on this rank's clients (BatchPlan._plan_poisson: a round
            # that drops one is outside the accounted mechanism; 0 in practice)
            rec["dp_lot_overflow"] = int(res.get("dp_lot_overflow", 0))
        return self.resolve_record(rec) if sync else rec

    def _set_params(self, new: torch.Tensor) -> None:
        """Update the global params IN PLACE: the trainer's cached round hipGraph reads them at a fixed address,
        so a fresh tensor per round (SecAgg / server-optimizer paths) would miss the graph cache every round."""
        self.params.copy_(new.to(self.params.dtype))

    def resolve_record(self, rec: dict) -> dict:
        """Read a round's metrics back (syncs with the device) and fill the derived fields."""
        if "_metrics" not in rec:
            return rec
        stamp = rec.pop("_out_stamp", None)
        if stamp is not None and self.epilogue.out_writes[stamp[0]] != stamp[1]:
            raise RuntimeError(f"round {rec['round']}: its metrics buffer was reused by a later round; resolve "
                               "records (resolve_record) within two rounds")
        m = rec.pop("_metrics").double().cpu().tolist()
        dt = time.perf_counter() - rec.pop("_t0")
        nrm = rec.pop("_norms", None)
        if nrm is not None:                      # CC6: every client's pre-clip update norm, clip fraction
            vals = nrm[0].double().cpu().numpy()[nrm[1]] if nrm[1] else np.zeros(0)
            if vals.size:
                C = self.cfg.privacy.clip_norm
                q = np.quantile(vals, [0.1, 0.5, 0.9])
                rec.update({"clip_frac": float((vals > C).mean()), "norm_p10": float(q[0]), "norm_p50": float(q[1]),
                            "norm_p90": float(q[2]),
                            "norms_private": False})   # raw, un-noised statistics (runtime.log_client_norms)
        if len(m) > 4 and m[4] > 0:
            raise RuntimeError(f"round {rec['round']}: {int(m[4])} fixed-point FedAvg terms saturated at 2^53 "
                               "(|w * Delta| > 2^21): lower the aggregation weights (train.weighting=uniform) or "
                               "the update magnitude (DP clipping / learning rate)")
        rec.update({"train_loss": m[0] / max(m[2], 1.0) if m[2] else float("nan"),
                    "train_acc": m[1] / max(m[2], 1.0) if m[2] else float("nan"),
                    "local_steps": int(round(m[3])), "round_time_s": dt,
                    "local_steps_per_s": m[3] / dt if dt > 0 else 0.0})
        return rec

    def run(self) -> dict:
        t = self.cfg.train
        self.maybe_resume()
        accs = []
        if self.start_round == 0:
            ev = self.evaluate()
            accs.append(ev["test_acc"])
            if self.world.is_main:
                self.log.info(f"Round 0: Test Accuracy = {ev['test_acc']:.4f}")
            self.metrics.log({"round": 0, **ev})
        else:
            accs = [h.get("test_acc") for h in self.history if "test_acc" in h]
        t_start = time.perf_counter()
        for r in range(self.start_round, t.num_rounds):
            rec = self.run_round(r)
            if (r + 1) % max(1, t.eval_every) == 0 or r + 1 == t.num_rounds:
                rec.update(self.evaluate())
                accs.append(rec["test_acc"])
            self.history.append(rec)
            self.metrics.log(rec)
            if self.world.is_main and ((r + 1) % self.cfg.runtime.log_every == 0 or r + 1 == t.num_rounds):
                eps = f" eps={rec['epsilon']:.3f}" if "epsilon" in rec else ""
                self.log.info(f"Round {r + 1}: Test Accuracy = {rec.get('test_acc', float('nan')):.4f} "
                              f"train_loss={rec['train_loss']:.4f} {rec['local_steps_per_s']:.1f} local-steps/s{eps}")
            ck = self.cfg.runtime.checkpoint_every
            if ck and (r + 1) % ck == 0:
                self.save(r + 1)
        wall = time.perf_counter() - t_start
        auc = self.test_auc()
        if self.world.is_main:
            self.metrics.log({"final": True, "test_auc": auc, "wall_s": wall})
        self.metrics.close()
        return {"model": self.adapter.state_dict(self.params), "params": self.params, "accuracies": accs,
                "auc": auc,
                "history": self.history, "wall_s": wall,
                # mean ms per TIMED round of each phase and how many rounds were timed (on the GPU only every
                # runtime.timer_every-th round is; raw totals would undercount the run by that factor)
                "phases_ms_per_round": self.timer.per_phase(), "phase_rounds_timed": dict(self.timer.counts),
                "epsilon": self.accountant.get_epsilon(self.cfg.privacy.delta) if self.cfg.privacy.dp else None}
