"""`GraphReplay`: replay of an algorithm's steady-state iteration from captured hipGraphs.

The mixin owns what is the same for every algorithm family: the side-stream warm-up, the capture (in segments around eager
collectives when a data-parallel run cannot record them), the unroll ladder, the fallback to eager launches, the launch census and
`graph_status()`. What an iteration IS -- its launches, its host bookkeeping, when it may be replayed -- comes from the algorithm
through the hooks declared at the end of the class. The mixin reads `device`, `world_size`, `learning_rate`, `n_envs`,
`num_timesteps`, `_total_timesteps` and `policy` of the algorithm and knows nothing about replay buffers, environments or noise.
"""
import gc
import math
import os
import sys
import warnings
from typing import Optional

import torch as th

from core import _native as nv
from core.common import distributed as dist_util
from core.common.callbacks import BaseCallback, to_callback

# Data-parallel runs under hipGraph replay. "auto" (default): record the RCCL all-reduces INTO the iteration's graph when a
# start-up trial (distributed.graph_collectives_ok: capture + replay of one all-reduce, result checked on every rank) passes,
# else run them eagerly BETWEEN graph segments; "0": always between segments; "1": always inside (no trial).
GRAPH_COLLECTIVES = os.environ.get("CSTR_GRAPH_COLLECTIVES", "auto")
GRAPH_WARMUP_ITERATIONS = 3


class GraphReplay:
    def _init_graph_state(self) -> None:
        """All graph state, once, from the algorithm's `__init__`."""
        self._graph_enabled = False
        self._graph: Optional[dict] = None       # cache key -> [CUDAGraph | eager callable, ...]; None: nothing recorded (yet / any more)
        self._graph_warm: dict = {}              # cache key -> warm-up iterations run so far
        self.graph_unroll = 1
        self._graph_error: Optional[str] = None  # text of the exception that ended hipGraph replay (None = never failed)
        self._graph_replays = 0                  # iterations served by a captured graph / by eager launches (bench.py reports both)
        self._eager_iterations = 0
        self._abi_launches: dict = {}            # phase -> C ABI launches recorded per iteration
        self._cap: Optional[dict] = None         # the recording in progress (pool, current graph, items)
        # both may be assigned from outside before enable_graph_capture: None = decided by `_collectives_in_graph`; True = give a
        # one-GPU run the launch structure of a data-parallel one (a boundary where each all-reduce would be)
        self._graph_collectives: Optional[bool] = None
        self._force_segment_boundaries = False
        self._graph_callback: Optional[BaseCallback] = None  # the callback of the iteration being decided (bounds the unroll)

    def enable_graph_capture(self, enabled: bool = True, unroll: Optional[int] = None) -> None:
        """Replay the steady-state iteration (actor forward, fused collect, `gradient_steps` gradient steps) from a
        captured hipGraph: ~250 launches become one host call. Every per-call control word the kernels need (ring
        position, Adam step, MT19937 stream, learning rate, env / RNG state) lives in HBM, so a replay is exact.
        Falls back to the eager path whenever the iteration is not capturable (warm-up, host-side action noise, episodic
        train_freq, a callback that has to see every step). A callback that knows its next event (`calls_until_event()`: the
        callbacks of core/common/callbacks.py) lets the iterations in between replay; the iteration that contains the event runs
        eagerly with the callback, so the hook fires where it always did.

        `unroll` (default 1, env CSTR_GRAPH_UNROLL): consecutive iterations recorded into ONE graph -- the ~10 us the GPU
        idles between two graph launches is paid once per `unroll` iterations. Used on one GPU, and data-parallel when the
        all-reduces are recorded into the graph (every rank replays the same graphs in the same order), with a constant learning
        rate while at least `unroll` iterations remain; the tail of a run replays graphs of unroll / 2, unroll / 4, ... 1 iterations."""
        self._graph_enabled = enabled
        self._graph, self._graph_error, self._abi_launches = None, None, {}
        self.graph_unroll = max(1, int(unroll if unroll is not None else os.environ.get("CSTR_GRAPH_UNROLL", "1")))

    def graph_status(self) -> dict:
        """What actually runs (not what was requested): bench.py refuses to report a run whose graphs fell back to eager."""
        graphs = self._graph if isinstance(self._graph, dict) else {}
        segs = [sum(isinstance(i, th.cuda.CUDAGraph) for i in items) for items in graphs.values()]
        mode = "none"
        if self._grads_need_allreduce():
            mode = "in-graph" if self._graph_collectives else "segmented"
        return dict(requested=bool(self._graph_enabled or self._graph_error), active=bool(self._graph_enabled and len(graphs) > 0),
                    graphs=len(graphs), segments_per_graph=segs, replays=self._graph_replays, eager_iterations=self._eager_iterations,
                    error=self._graph_error, graph_collectives=mode,
                    abi_launches_per_iteration={int(k): v for k, v in sorted(self._abi_launches.items())})

    # ---- one iteration ---------------------------------------------------------------------------------------------
    def _learn_iteration(self, callback: BaseCallback, log_interval: Optional[int]) -> bool:
        """One iteration of learn() (False: the callback ends training): replayed from a captured hipGraph when it is eligible (same
        launches, same order, one host call), launched eagerly otherwise."""
        self._graph_callback = callback
        if self._graph_enabled and self._graph_eligible(callback):
            self._graph_iteration(log_interval, callback)
            return True
        self._eager_iterations += 1
        return self._eager_iteration(callback, log_interval)

    def _graph_calls_per_iteration(self) -> int:
        """`callback.on_step()` calls one body stands for: its vec-steps."""
        return max(self._graph_steps_per_iteration() // max(self.n_envs, 1), 1)

    def _graph_skippable_calls(self, callback: Optional[BaseCallback]) -> float:
        """How many coming `on_step()` calls the callback declares eventless (inf: all of them; 0: it has to see every step)."""
        if callback is None or getattr(callback, "is_noop", False):
            return math.inf
        k = callback.calls_until_event()
        return 0 if k is None else k - 1

    def _callback_allows_replay(self, callback: BaseCallback) -> bool:
        """The coming iteration may run without its callback: a no-op callback, or one whose next event lies behind the iteration."""
        return self._graph_skippable_calls(callback) >= self._graph_calls_per_iteration()

    def _graph_unroll_now(self) -> int:
        u = self.graph_unroll
        if u <= 1 or not isinstance(self.learning_rate, float):
            return 1
        if self._grads_need_allreduce() and not self._collectives_in_graph():
            return 1  # data-parallel with the collectives BETWEEN graph segments: one iteration per replay list
        remaining = (self._total_timesteps - self.num_timesteps) // self._graph_steps_per_iteration()
        # ... and the callback's next event: the bodies of one graph must all lie in front of it
        skippable = self._graph_skippable_calls(self._graph_callback)
        if skippable != math.inf:
            remaining = min(remaining, int(skippable) // self._graph_calls_per_iteration())
        while u > 1 and remaining < u:  # the tail of a run: the largest of u, u / 2, u / 4, ... that still fits
            u //= 2
        return max(u, 1)

    def _graph_iteration(self, log_interval: Optional[int], callback: Optional[BaseCallback] = None) -> None:
        opt = getattr(getattr(self.policy, "actor", None), "optimizer", None)
        if getattr(opt, "shadow", None) is not None:  # torch changed the actor's weights (a callback, load_state_dict): the
            opt.refresh_shadow(force=False)           # replayed graph reads their tile-major copy -- one version compare
        unroll = self._graph_unroll_now()
        key = self._graph_cache_key(unroll)
        if self._graph is None:
            self._graph, self._graph_warm = {}, {}
        if key not in self._graph:
            # side-stream warm-up (these are REAL iterations: they advance env, ring, RNG and optimiser state)
            warm = self._graph_warm.get(key, 0)
            if warm < GRAPH_WARMUP_ITERATIONS:
                self._graph_host_pre()
                side = th.cuda.Stream(device=self.device)
                side.wait_stream(th.cuda.current_stream(self.device))
                with th.cuda.stream(side):
                    self._graph_body()
                th.cuda.current_stream(self.device).wait_stream(side)
                self._graph_warm[key] = warm + 1
                self._eager_iterations += 1
                self._graph_host_bookkeeping(log_interval)
                self._skip_callback_calls(callback, 1)
                return
            self._graph_host_pre()
            try:
                self._graph[key] = self._capture_segments(unroll)
            except Exception as exc:  # something in the iteration is not capturable: run eagerly from now on
                self._graph_error = f"{type(exc).__name__}: {exc}"
                warnings.warn(f"hipGraph capture failed ({self._graph_error}); falling back to eager launches")
                self._graph_enabled, self._graph = False, None
                self._learn_iteration(callback if callback is not None else self._noop_callback(), log_interval)
                return
        self._graph_host_pre()
        for item in self._graph[key]:  # hipGraph segments interleaved with the eager collectives that separate them
            item.replay() if isinstance(item, th.cuda.CUDAGraph) else item()
        self._graph_replays += unroll
        for _ in range(unroll):
            self._graph_host_bookkeeping(log_interval)
        self._skip_callback_calls(callback, unroll)

    def _skip_callback_calls(self, callback: Optional[BaseCallback], bodies: int) -> None:
        """`bodies` iterations ran on the device without their callback (which had declared them eventless): count them."""
        if callback is not None and not getattr(callback, "is_noop", False):
            callback.skip_calls(bodies * self._graph_calls_per_iteration())

    def _noop_callback(self) -> BaseCallback:
        cb = to_callback(None)
        cb.init_callback(self)
        return cb

    # ---- recording -------------------------------------------------------------------------------------------------
    def _capture_segments(self, unroll: int = 1) -> list:
        """`_record_segments`, and if recording WITH the collectives inside the graph raises (every rank runs the same code,
        so every rank gets here), once more with the collectives between graph segments."""
        try:
            return self._record_segments(unroll)
        except Exception as exc:  # noqa: BLE001
            if not (self.world_size > 1 and self._graph_collectives and GRAPH_COLLECTIVES == "auto"):
                raise
            print(f"[graph] recording the collectives into the graph failed ({exc!r}); keeping them between graph segments", file=sys.stderr)
            self._graph_collectives = False
            th.cuda.synchronize(self.device)
            return self._record_segments(unroll)

    def _record_segments(self, unroll: int = 1) -> list:
        """Record the iteration as hipGraph segments. A data-parallel run has an RCCL all-reduce between backward and
        the optimiser step (two per SAC gradient step). When the start-up trial passes (`_collectives_in_graph`) they are
        recorded into the graph; otherwise collectives stay OUTSIDE the captured graphs -- every `_eager_boundary` closes the
        current segment, runs the collective eagerly and opens the next segment in the same memory pool (activations saved
        for a later segment's backward stay alive). Single-GPU runs have no boundary and get one graph."""
        # like torch.cuda.graph(): collect garbage BEFORE recording and keep the collector off while recording -- a cycle
        # collection that destroys another model's CUDAGraph (or frees device memory) in the middle of a capture aborts
        self._collectives_in_graph()  # decided (start-up trial, world > 1) before anything is being recorded
        gc.collect()
        gc_was_enabled = gc.isenabled()
        gc.disable()
        th.cuda.synchronize(self.device)
        side = th.cuda.Stream(device=self.device)
        side.wait_stream(th.cuda.current_stream(self.device))
        items: list = []
        with th.cuda.stream(side):
            self._cap = dict(pool=th.cuda.graph_pool_handle(), graph=th.cuda.CUDAGraph(), items=items)
            self._cap["graph"].capture_begin(pool=self._cap["pool"], capture_error_mode="thread_local")
            recorded = 0
            calls0 = nv.ABI_CALLS[0]
            try:
                for _ in range(unroll):
                    self._graph_body()
                    self._graph_shift_phase(1)  # the next body sees its own policy-delay phase
                    recorded += 1
                self._cap["graph"].capture_end()
                items.append(self._cap["graph"])
                # launches recorded per iteration of this policy-delay phase (every launch of the captured body goes through the
                # C ABI; bench.py reports it, tools/count_launches.sh is the rocprofv3 cross-check)
                self._abi_launches[self._graph_phase()] = (nv.ABI_CALLS[0] - calls0) / unroll
            except Exception:
                try:  # leave capture mode before the graph object is destroyed
                    self._cap["graph"].capture_end()
                except Exception:
                    pass
                # nothing of the recorded body ran: host-side debts of the one-launch rollout (indices "drawn" by a launch that was
                # only recorded, a Philox advance handed to a consumer that was never reached) must not reach the eager fallback
                self._drop_recording_debts()
                raise
            finally:
                self._cap = None
                self._graph_shift_phase(-recorded)  # nothing ran while recording
                if gc_was_enabled:
                    gc.enable()
        th.cuda.current_stream(self.device).wait_stream(side)
        th.cuda.synchronize(self.device)
        return items

    # ---- collectives -----------------------------------------------------------------------------------------------
    def _collectives_in_graph(self) -> bool:
        if self._graph_collectives is None:
            if GRAPH_COLLECTIVES in ("0", "1"):
                self._graph_collectives = GRAPH_COLLECTIVES == "1"
            else:
                self._graph_collectives = self.world_size > 1 and dist_util.graph_collectives_ok(self.device)
        return self._graph_collectives

    def _eager_boundary(self, fn) -> None:
        """Run `fn` (a collective) eagerly; when a capture is in progress, split the graph around it."""
        cap = self._cap
        if cap is None or self._collectives_in_graph():
            # no capture in progress, or the collective is recorded into the graph like any other launch (RCCL issues a
            # blocking collective on the current stream) and the iteration stays ONE graph
            fn()
            return
        cap["graph"].capture_end()
        cap["items"].append(cap["graph"])
        fn()
        cap["items"].append(fn)
        cap["graph"] = th.cuda.CUDAGraph()
        cap["graph"].capture_begin(pool=cap["pool"], capture_error_mode="thread_local")

    def _grads_need_allreduce(self) -> bool:
        """A collective (or the segment boundary that stands in for one) separates every gradient from its optimiser step."""
        return self.world_size > 1 or self._force_segment_boundaries

    def _allreduce_grads(self, arena) -> None:
        """The data-parallel helper of train(): sum `arena`'s gradient over the ranks (the optimisers scale by 1 / world_size)."""
        if self._grads_need_allreduce():
            buf = getattr(arena, "grad_full", None)
            buf = arena.grad if buf is None else buf
            self._eager_boundary(lambda: dist_util.allreduce_sum_(buf))

    # ---- hooks: what the algorithm supplies ------------------------------------------------------------------------
    def _graph_eligible(self, callback: BaseCallback) -> bool:
        """Whether the coming iteration is exactly what `_graph_body` launches (else it runs eagerly)."""
        raise NotImplementedError

    def _graph_cache_key(self, unroll: int) -> tuple:
        """What a captured graph depends on besides the device state it reads (one graph per distinct key); `unroll` comes last."""
        raise NotImplementedError

    def _graph_body(self) -> None:
        """Every device launch of one iteration and nothing that syncs; looked up on the instance at every use."""
        raise NotImplementedError

    def _graph_host_bookkeeping(self, log_interval: Optional[int]) -> None:
        """The host side of one iteration that ran on the device (counters, progress, logger records)."""
        raise NotImplementedError

    def _graph_steps_per_iteration(self) -> int:
        """Env steps one body advances `num_timesteps` by (the unroll ladder counts the bodies that still fit into the run)."""
        return self.n_envs

    def _graph_phase(self) -> int:
        """Which of the alternating launch sequences the coming iteration is (a delayed policy update: one graph per residue)."""
        return 0

    def _graph_shift_phase(self, iterations: int) -> None:
        """Move `_graph_phase` by `iterations` bodies (negative: back) without running anything: unrolled bodies are recorded in turn."""
        raise NotImplementedError

    def _train_host_pre(self) -> None:
        """The host prologue of train() (learning-rate schedule), run before every warm-up, capture and replay."""
        raise NotImplementedError

    def _graph_host_pre(self) -> None:
        """What the host does before every warm-up body, capture and replay; by default train()'s own prologue."""
        self._train_host_pre()

    def _drop_recording_debts(self) -> None:
        """Forget host-side promises made by launches that were only recorded, after a recording failed."""
        raise NotImplementedError

    def _eager_iteration(self, callback: BaseCallback, log_interval: Optional[int]) -> bool:
        """The iteration as eager launches, callbacks included; False ends training."""
        raise NotImplementedError
