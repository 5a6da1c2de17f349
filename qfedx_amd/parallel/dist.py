"""Process-group runtime: one process per GPU, RCCL over xGMI (backend "nccl" on ROCm), gloo on CPU.

Reference: no collectives at all - aggregation is an in-process loop over state_dicts
(``Classical_FL.py:66-81``) and clients run sequentially (``:132-140``); the ROADMAP plans Ray /
MPI / Slurm (``ROADMAP.md:39,77-89``).  Design here:

* clients are sharded over ranks in contiguous blocks; each GPU reduces ITS clients locally first
  (fixed client order), so every round sends exactly one P-sized message per rank (CC2);
* the update sum, sum of weights and the round metrics travel in ONE flat buffer -> one
  all-reduce per round (CC2+CC3), latency-bound on xGMI (<= 0.5 MB), so fewer/larger messages;
* ``exact`` mode all-reduces a fixed-point int64 encoding: integer sums are associative, so the
  aggregate is bitwise identical for 1/2/4/8 ranks;
* the round's collective and the in-place apply are captured into the round's hipGraph with the local steps
  (``fl/round_graph.py`` ``RoundGraph.capture``; RCCL accepts capture), so a round is one graph launch with no host
  round trip between training and aggregation.  Nothing of round r + 1 can overlap the collective: its local
  steps start from the theta the collective produces, and the theta-independent part (the minibatch gather of the
  round prologue) is a few microseconds.  A comm-stream / layer-bucket overlap design was removed in round 3 as
  dead code for that reason: the one message per round is <= 1 MB (TinyCNN, 911 KB as int64), latency-bound on
  xGMI, so bucketing would only add launches (CC4);
* ``ShardedServerState``: reduce-scatter + all-gather for a server optimizer whose state is
  sharded P/world per rank (CC5).
"""
from __future__ import annotations

import datetime
import os
from dataclasses import dataclass
from typing import Callable, Optional

import torch
import torch.distributed as dist


_OWN_PORT: list = []     # MASTER_PORT values picked here for single-rank groups


@dataclass
class World:
    rank: int = 0
    world_size: int = 1
    local_rank: int = 0
    backend: str = "none"
    device: torch.device = torch.device("cpu")

    @property
    def is_main(self) -> bool:
        return self.rank == 0

    @property
    def distributed(self) -> bool:
        """A process group exists: collectives run through it (also for ONE rank when a backend was named)."""
        return self.backend != "none"


def init_distributed(device: torch.device, backend: str = "auto", timeout_s: int = 600) -> World:
    """This process's place in the job.  WORLD_SIZE > 1 (torchrun) always creates the process group; at
    WORLD_SIZE = 1 a group is created only when ``backend`` is named explicitly ("nccl" / "gloo"): a
    single-rank RCCL communicator then runs every collective of the round exactly as in an 8-GPU job (the
    GPU tests use it to exercise the RCCL path on a one-GPU box); "auto" at one rank skips the group."""
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    if ws <= 1 and backend == "auto":
        return World(0, 1, 0, "none", device)
    if backend == "auto":
        backend = "nccl" if device.type == "cuda" else "gloo"
    if backend == "nccl" and device.type != "cuda":
        raise ValueError("dist_backend=nccl (RCCL) needs a GPU device")
    if backend == "nccl":
        # RCCL runs one rank per GPU: more local ranks than visible GPUs would put two ranks on one device (the
        # device map takes LOCAL_RANK modulo the count) and fail deep inside communicator setup.  device_count()
        # does not initialise the GPU.
        # Only what the launcher actually set is checked: a multi-node srun / mpirun job that sets RANK and
        # WORLD_SIZE but no LOCAL_* variables has no local-rank information to check against (the global RANK
        # is not a local index there).
        ngpu = torch.cuda.device_count()
        lws = int(os.environ["LOCAL_WORLD_SIZE"]) if "LOCAL_WORLD_SIZE" in os.environ else 0
        lrank = int(os.environ["LOCAL_RANK"]) if "LOCAL_RANK" in os.environ else -1
        if lrank >= ngpu or lws > ngpu:
            raise RuntimeError(f"dist_backend=nccl (RCCL) needs one GPU per rank: LOCAL_RANK={local} of "
                               f"{lws} local ranks, but {ngpu} GPU(s) visible; launch at most {ngpu} ranks per node "
                               "or use dist_backend=gloo")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:
        if ws > 1:
            os.environ["MASTER_PORT"] = "29500"
        else:                               # a private single-rank group: any free local port
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            _OWN_PORT.append(os.environ["MASTER_PORT"])
    if not dist.is_initialized():
        kw = {}
        if backend == "nccl" and device.type == "cuda":
            kw["device_id"] = device
        dist.init_process_group(backend=backend, rank=rank, world_size=ws,
                                timeout=datetime.timedelta(seconds=timeout_s), **kw)
    return World(rank, ws, local, backend, device)


def shutdown(world: World) -> None:
    if world.distributed and dist.is_initialized():
        dist.destroy_process_group()
    while _OWN_PORT:                          # the private single-rank port is not reused by a later group
        if os.environ.get("MASTER_PORT") == _OWN_PORT.pop():
            os.environ.pop("MASTER_PORT", None)


def shard_clients(num_clients: int, world_size: int, rank: int) -> list[int]:
    """Contiguous block of client ids for ``rank`` (sizes differ by at most one)."""
    base, rem = divmod(num_clients, world_size)
    start = rank * base + min(rank, rem)
    return list(range(start, start + base + (1 if rank < rem else 0)))


def barrier(world: World) -> None:
    if world.distributed:
        if world.backend == "nccl":
            dist.barrier(device_ids=[world.device.index])
        else:
            dist.barrier()


def all_reduce_(t: torch.Tensor, world: World, op=None) -> torch.Tensor:
    if world.distributed:
        dist.all_reduce(t, op=op or dist.ReduceOp.SUM)
    return t


class _Done:
    def wait(self):
        return True

    def is_completed(self):
        return True


def all_reduce_async(t: torch.Tensor, world: World, op=None):
    """Issue the SUM all-reduce of ``t`` and return a handle whose ``wait()`` completes it (CC4: the caller does the
    next round's theta-independent work in between).  gloo runs the collective on its own worker thread, so host
    work overlaps it; RCCL enqueues it on the current stream (the device-side overlap is the trainer's side stream,
    fl/trainer.py ``RoundPrefetch``).  Single process: a completed handle."""
    if not world.distributed:
        return _Done()
    return dist.all_reduce(t, op=op or dist.ReduceOp.SUM, async_op=True)


def broadcast_(t: torch.Tensor, world: World, src: int = 0) -> torch.Tensor:
    if world.distributed:
        dist.broadcast(t, src)
    return t


def all_gather_cat(t: torch.Tensor, world: World) -> torch.Tensor:
    """All-gather variable-length 1-D tensors (e.g. per-client norms, CC6)."""
    if not world.distributed:
        return t
    n = torch.tensor([t.numel()], device=t.device, dtype=torch.int64)
    sizes = [torch.zeros_like(n) for _ in range(world.world_size)]
    dist.all_gather(sizes, n)
    mx = int(max(int(s) for s in sizes))
    pad = torch.zeros(mx, dtype=t.dtype, device=t.device)
    pad[: t.numel()] = t.reshape(-1)
    outs = [torch.zeros_like(pad) for _ in range(world.world_size)]
    dist.all_gather(outs, pad)
    return torch.cat([o[: int(s)] for o, s in zip(outs, sizes)])


def max_over_ranks(x: float, world: World, device=None) -> float:
    if not world.distributed:
        return x
    t = torch.tensor([x], dtype=torch.float64, device=device or world.device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def reduce_scatter_(full: torch.Tensor, world: World) -> torch.Tensor:
    """Sum ``full`` [world * chunk] over ranks and return this rank's chunk (CC5).  gloo has no
    reduce-scatter: there it is an all-reduce + slice (same result, CPU test path)."""
    ws = world.world_size
    chunk = full.numel() // ws
    if not world.distributed:
        return full[:chunk].clone()
    if world.backend == "gloo":
        buf = full.clone()
        dist.all_reduce(buf)
        return buf[world.rank * chunk: (world.rank + 1) * chunk].clone()
    out = torch.empty(chunk, dtype=full.dtype, device=full.device)
    dist.reduce_scatter_tensor(out, full.contiguous())
    return out


def all_gather_(shard: torch.Tensor, world: World) -> torch.Tensor:
    """Concatenate every rank's equally sized ``shard`` (CC5)."""
    if not world.distributed:
        return shard.clone()
    out = torch.empty(shard.numel() * world.world_size, dtype=shard.dtype, device=shard.device)
    if world.backend == "gloo":
        parts = [torch.empty_like(shard) for _ in range(world.world_size)]
        dist.all_gather(parts, shard.contiguous())
        return torch.cat(parts)
    dist.all_gather_into_tensor(out, shard.contiguous())
    return out


class ShardedServerState:
    """Server-side optimizer over the aggregated update with its state sharded P/world per rank (CC5).

    ``kind``: ``fedavg`` (theta += lr * mean update), ``momentum`` (FedAvgM, v = beta v + d) or ``adam``
    (FedAdam, Reddi et al. 2021: m, v moments, tau adaptivity).  The input is the EXACT int64 fixed-point
    sum of the clients' weighted updates (scale 2^32): it is reduce-scattered (integer sums are
    associative -> rank-count invariant), each rank steps its slice in float64, and the new parameter
    slices are all-gathered.
    """

    def __init__(self, P: int, world: World, device, kind: str = "momentum", lr: float = 1.0,
                 momentum: float = 0.9, betas=(0.9, 0.99), tau: float = 1e-3, scale: float = 2.0 ** 32):
        self.world = world
        self.P = P
        ws = world.world_size
        self.chunk = (P + ws - 1) // ws
        self.padded = self.chunk * ws
        self.kind = kind
        self.lr = lr
        self.momentum = momentum
        self.b1, self.b2 = betas
        self.tau = tau
        self.scale = scale
        self.t = 0
        self.m = torch.zeros(self.chunk, dtype=torch.float64, device=device)
        self.v = torch.zeros(self.chunk, dtype=torch.float64, device=device) if kind == "adam" else None

    def step(self, global_params: torch.Tensor, update_sum_fixed: torch.Tensor, wsum: torch.Tensor) -> torch.Tensor:
        """``update_sum_fixed``: this rank's int64 [P] fixed-point weighted update sum; ``wsum``: the
        all-reduced weight total (0-d tensor).  Returns the new full parameter vector."""
        dev = update_sum_fixed.device
        flat = torch.zeros(self.padded, dtype=torch.int64, device=dev)
        flat[: self.P] = update_sum_fixed
        shard = reduce_scatter_(flat, self.world).double() / self.scale
        d = shard / wsum.to(dev).double().clamp(min=1e-300)
        self.t += 1
        if self.kind == "momentum":
            self.m.mul_(self.momentum).add_(d)
            step = self.lr * self.m
        elif self.kind == "adam":
            self.m.mul_(self.b1).add_((1 - self.b1) * d)
            self.v.mul_(self.b2).add_((1 - self.b2) * d * d)
            step = self.lr * self.m / (self.v.sqrt() + self.tau)
        else:
            step = self.lr * d
        step = torch.where(wsum.to(dev) > 0, step, torch.zeros_like(step))
        full = all_gather_(step, self.world)
        return (global_params.double() + full[: self.P]).to(global_params.dtype)

    def state_dict(self) -> dict:
        """Full (un-sharded) optimizer state, identical on every rank.  COLLECTIVE: every rank calls it
        (the moment shards are all-gathered), so the checkpoint resumes at any world size."""
        def full(x):
            return all_gather_(x, self.world)[: self.P].cpu()
        empty = torch.zeros(0, dtype=torch.float64)
        return {"kind": self.kind, "t": torch.tensor(self.t, dtype=torch.int64), "m": full(self.m),
                "v": full(self.v) if self.v is not None else empty}

    def load_state_dict(self, sd: dict) -> None:
        """Restore from :meth:`state_dict` (any saving world size): this rank keeps its own P/world slice."""
        if sd.get("kind", self.kind) != self.kind:
            raise ValueError(f"checkpoint server optimizer {sd.get('kind')!r} != configured {self.kind!r}")
        self.t = int(sd["t"])
        lo = self.world.rank * self.chunk

        def shard(x):
            pad = torch.zeros(self.padded, dtype=torch.float64)
            pad[: self.P] = x.double().reshape(-1)[: self.P]
            return pad[lo: lo + self.chunk].to(self.m.device)
        self.m = shard(sd["m"])
        if self.v is not None:
            self.v = shard(sd["v"])


def graph_allreduce_selfcheck(world: World) -> Optional[Callable[[], bool]]:
    """This rank's half of the captured-collective self-check: capture ONE all-reduce of a rank-dependent int64
    buffer into a hipGraph.  Returns a callable that replays it and compares the result bitwise with an eager
    all-reduce of the same buffer, or None when capture failed here.  The replay may only run once every rank has
    captured (``agree_graph_comm``): a replay on some ranks alone would wait forever for the others."""
    dev = world.device
    x = torch.arange(4096, dtype=torch.int64, device=dev) * 7 + (world.rank + 1) * 1_000_003
    try:
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):            # warm-up outside capture (communicator set up for this stream)
            w = x.clone()
            dist.all_reduce(w)
        torch.cuda.current_stream(dev).wait_stream(side)
        static = torch.zeros_like(x)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            dist.all_reduce(static)
    except Exception:
        return None

    def replay_and_compare() -> bool:
        eager = x.clone()
        dist.all_reduce(eager)
        static.copy_(x)
        g.replay()
        torch.cuda.synchronize(dev)
        return bool(torch.equal(static, eager))
    return replay_and_compare


def _vote(ok: bool, world: World) -> bool:
    """True iff every rank voted True (one eager MIN all-reduce)."""
    if not world.distributed:
        return ok
    t = torch.tensor([1 if ok else 0], dtype=torch.int64,
                     device=world.device if world.backend == "nccl" else torch.device("cpu"))
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(int(t.item()))


def agree_graph_comm(world: World, want: bool, probe=graph_allreduce_selfcheck) -> bool:
    """Rank-agreed decision whether the round's collective is captured into the round hipGraph (CC2 on RCCL).

    ``want`` must be the same on every rank (it comes from the shared config).  Each rank captures one all-reduce
    (``probe``); the ranks vote, and only if ALL captured do they replay it and compare it bitwise with an eager
    all-reduce, then vote again.  So either every rank captures its round collective or none does: a rank that
    cannot capture never leaves the others replaying a collective it runs eagerly at another point of its stream.
    Without a process group there is no collective in the graph and nothing to check."""
    if not want:
        return False
    if not world.distributed:
        return True
    replay = probe(world)
    if not _vote(replay is not None, world):
        return False
    # a replay that raises on one rank must still reach the second vote, or the other ranks block in it forever
    try:
        ok = bool(replay())
    except Exception:                       # noqa: BLE001 - any failure means: do not capture the collective
        ok = False
    return _vote(ok, world)
