"""The captured round: one federated round of a rank's clients as a hipGraph (``RoundGraph``), the key a captured
shape is cached under (``graph_key``), the LRU of captured shapes (``GraphLRU``) and the context the trainer hands
to the round epilogue (``RoundCtx``).  ``fl/trainer.py`` decides when a round is graphed and runs the local steps."""
from __future__ import annotations

import time
import warnings
from collections import OrderedDict, namedtuple
from dataclasses import dataclass
from typing import Optional

import torch

WAIT_S = [0.0]     # host seconds spent waiting for the GPU in wait_uploads (bench: host enqueue cost = loop - wait)


@dataclass
class RoundCtx:
    """What the trainer tells the round epilogue (``reduce`` / ``fused_tail``) about the call it is making."""
    variant: Optional[int] = None     # capture: post(variant) follows right behind the reduce, in the same graph
    eager: bool = False               # not captured: the caller runs post (if any) itself, after run_round
    fed_done: bool = False            # the engine's last local step already ran the FedAvg (fused_tail)


GraphKey = namedtuple("GraphKey", "clients steps batch nmax store_ptr tables theta_ptr epilogue post cc4")


def graph_key(store, plan, tabs: dict, theta_g: torch.Tensor, epilogue, post, cc4: bool) -> GraphKey:
    """The cache key of a round graph (``theta_ptr``: the global params when read in place, else None: copied into a
    static buffer per round).  A capture FREEZES what the key names and everything the trainer, ``epilogue`` and
    ``post`` computed on the host while captured: their launches, scalar arguments (learning rate, clip norm, round
    number, client ids) and buffers; a host value that changes between rounds and is not in the key stays what the
    capture saw.  PER ROUND travel only the upload (``PackedUpload``: client slots, minibatch indices, loss weights,
    step masks, FedAvg weights, every ``extra`` per-client table) and the global params, through their address."""
    direct = theta_g.is_cuda and theta_g.dtype == torch.float32 and theta_g.is_contiguous()
    return GraphKey(int(tabs["lid"].shape[0]), plan.max_steps, plan.B, store.nmax, store.X.data_ptr(), tuple(tabs),
                    theta_g.data_ptr() if direct else None, epilogue is not None, post is not None, cc4)


class SideGather:
    """CC4 state of one round graph: the round's upload and minibatch gather run on a side stream, into per-variant
    minibatch buffers, ordered by events against the graph that last read that variant."""

    def __init__(self, key: GraphKey, F: int, P: int, dev):
        K, S, B = key.clients, key.steps, key.batch
        self.xy = [(torch.empty(S, K, B, F, dtype=torch.float32, device=dev),
                    torch.empty(S * K * B, dtype=torch.int64, device=dev)) for _ in range(2)]
        self.stream = torch.cuda.Stream(device=dev)
        self.ev_g = [torch.cuda.Event() for _ in range(2)]      # variant v's gather is done
        self.ev_c = [torch.cuda.Event() for _ in range(2)]      # variant v's graph is done (once recorded: c_rec)
        self.c_rec = [False, False]
        self.pshape = torch.empty(K, P, dtype=torch.float32, device=dev)   # row-less prologue: shape only


class RoundGraph:
    """One captured round shape, in two variants that differ only in the pinned host buffer their first node reads
    the round's packed tables from: replay n fills pinned buffer n % 2 - free once replay n - 2's upload has
    finished - and replays variant n % 2, so the host stays a round ahead with no upload launch of its own."""

    def __init__(self, trainer, store, up, theta_g: torch.Tensor, key: GraphKey):
        from ..ops._ext import ext
        E = ext()
        dev = trainer.device
        self.trainer, self.store, self.key = trainer, store, key
        # static device tables (views of ``packs``): one set per variant with CC4, else one
        self.packs: list = [torch.empty(up.nbytes, dtype=torch.uint8, device=dev) for _ in range(2 if key.cc4 else 1)]
        self.tables: list = [up.to_device(dev, pk) for pk in self.packs]
        # the global params themselves (read in place), or a static copy
        self.theta: torch.Tensor = theta_g if key.theta_ptr is not None else theta_g.to(dev).float().clone()
        self.pin: list = [E.host_alloc(up.nbytes), E.host_alloc(up.nbytes)]
        # upload-completion counter (round count + block arrivals) and its coherent host word, both written by the
        # graph's first node (the upload kernel's last block)
        self.ctr: torch.Tensor = torch.zeros(2, dtype=torch.int64, device=dev)
        self.flag: torch.Tensor = E.host_alloc(8, True)
        self.flag.zero_()
        self.launched = self.flip = 0           # replays so far; the next variant
        self.side: Optional[SideGather] = None  # present with CC4 only
        if key.cc4:
            self.side = SideGather(key, store.X.shape[-1], theta_g.numel(), dev)
        self.ws: dict = {}                      # the graphs own their workspaces: eager calls never regrow / free them
        self.graphs, self.out = [], []          # the two graphs and their static outputs (params, loss, correct)
        self.post_in_graph: bool = False        # post(v) is captured behind the epilogue (else: run after the replay)

    def tabs(self, v: int) -> dict:
        return self.tables[v if self.side is not None else 0]

    def upload_job(self, v: int, nbytes: int) -> tuple:
        """The host upload of variant v: pinned source, device destination, counter, host word."""
        return self.pin[v][:nbytes], self.packs[v if self.side is not None else 0], self.ctr, self.flag

    def _round(self, v: int, epilogue, ctx: RoundCtx, round_num: int, upload=None):
        return self.trainer._round(self.store, self.tabs(v), self.theta, self.key.steps, round_num, "adjoint",
                                   epilogue, ctx, xy=self.side.xy[v] if self.side is not None else None,
                                   upload=upload)

    def _capture(self, up, epilogue, post, round_num: int) -> None:
        """Both variants: fill pinned buffer v, then capture variant v - the upload (in the graph without CC4), the
        local steps, the epilogue and, when given, ``post(v)`` right behind it."""
        self.graphs, self.out, self.post_in_graph = [], [], post is not None
        for v in range(2):
            up._fill(self.pin[v][: up.nbytes])
            g = torch.cuda.CUDAGraph()
            # thread-local capture: the RCCL watchdog thread queries its work events at any time, and in the global
            # mode such a query during the capture aborted the process (hipErrorStreamCaptureUnsupported, seen once
            # in tests/test_gpu_rccl.py)
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                out = self._round(v, epilogue, RoundCtx(variant=v if post is not None else None), round_num,
                                  upload=self.upload_job(v, up.nbytes) if self.side is None else None)
                if post is not None:
                    post(v)
            self.graphs.append(g)
            self.out.append(out)

    def capture(self, up, epilogue, post, round_num: int) -> None:
        """Warm up eagerly on a side stream (no collective / apply: modules loaded, sizes fixed), then capture both
        variants, with ``post`` inside when the trainer's ``graph_comm`` allows it."""
        tr, dev = self.trainer, self.trainer.device
        cur = torch.cuda.current_stream(dev)
        with tr.engine.hip.private_workspace(self.ws):
            warm = torch.cuda.Stream(device=dev)
            warm.wait_stream(cur)
            with torch.cuda.stream(warm):
                if self.side is not None:   # gather only, from the device tables to_device filled (no pinned upload)
                    tr._cc4_gather(self, up, 0, wait=False, upload=False)
                self._round(0, epilogue, RoundCtx(), round_num)
            cur.wait_stream(warm)
            in_graph = post is not None and tr.graph_comm
            try:
                self._capture(up, epilogue, post if in_graph else None, round_num)
            except Exception as exc:
                if not in_graph:
                    raise
                # the collective refused capture although the ranks agreed it could be captured (parallel/dist.py
                # agree_graph_comm): graphs without it, post() runs eagerly right after the replay - the same point
                # of this rank's collective sequence, so ranks stay matched
                warnings.warn(f"round collective capture failed ({exc!r}); running it eagerly on this rank")
                tr.capture_fallbacks += 1
                tr.graph_comm = False
                torch.cuda.synchronize(dev)
                self._capture(up, epilogue, None, round_num)

    def replay(self, up) -> int:
        """Feed and launch the next variant; returns it."""
        v = self.flip
        self.flip ^= 1
        n = self.launched
        self.wait_uploads(n - 1)                    # pinned buffer v: its last reader (replay n - 2) is done
        up._fill(self.pin[v][: up.nbytes])
        side = self.side
        if side is not None:
            # side stream: this round's upload + gather, behind only the graph that last read variant v's buffers
            # (round r - 2); it runs while round r - 1's graph, collective included, is still on the main stream
            self.trainer._cc4_gather(self, up, v)
            torch.cuda.current_stream(self.trainer.device).wait_event(side.ev_g[v])
        self.graphs[v].replay()
        if side is not None:
            side.ev_c[v].record(torch.cuda.current_stream(self.trainer.device))
            side.c_rec[v] = True
        self.launched = n + 1
        return v

    def wait_uploads(self, n: int) -> None:
        """Block until the uploads of ``n`` replays have finished (the round's first node, the upload kernel, publishes
        the count to the coherent pinned word once every block has read its pinned buffer): spins briefly, then
        yields; the GPU is normally far ahead of this."""
        if n <= 0:
            return
        flag = self.flag.view(torch.int64)
        if int(flag[0]) >= n:
            return
        spins, t0, tw = 0, None, time.perf_counter()
        while int(flag[0]) < n:
            spins += 1
            if spins > 64:
                time.sleep(20e-6)
                if t0 is None:
                    t0 = time.perf_counter()
                elif time.perf_counter() - t0 > 5.0:     # never expected: drain the GPU, then the word must be there
                    torch.cuda.synchronize()
                    if int(flag[0]) < n:
                        raise RuntimeError(f"round signal stuck at {int(flag[0])} < {n}: device writes to the "
                                           "coherent pinned word are not visible to the host")
        WAIT_S[0] += time.perf_counter() - tw

    def drain(self) -> None:
        """The counter only says the uploads are done: drain the device too before the graphs and their workspaces
        are released."""
        self.wait_uploads(self.launched)
        torch.cuda.current_stream(self.trainer.device).synchronize()


class GraphLRU(OrderedDict):
    """The live round graphs by key, most recently used last.  Inserting past ``capacity`` drains the oldest entry
    (``drain()``) and then drops it (rare: more live shapes than the cache holds)."""

    def __init__(self, capacity: int):
        super().__init__()
        self.capacity = capacity

    def get(self, key):
        """The entry of ``key`` (now the most recently used), or None."""
        if key not in self:
            return None
        self.move_to_end(key)
        return self[key]

    def put(self, key, ent) -> None:
        while len(self) >= self.capacity:
            old = next(iter(self))
            self[old].drain()
            del self[old]
        self[key] = ent
