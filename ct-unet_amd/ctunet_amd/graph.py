"""Whole-step HIP graph: forward + loss + backward + optimizer of one fixed-shape batch, captured once
and replayed, so the ~270 kernel launches of a step cost one graph launch (MI355X guide: "capture
launch-bound inner loops in hipGraphs").

The step is the reference's ``Model.forward_pass`` train branch (ctunet/pytorch/Model.py:343-374) minus its
host round trips: the per-term ``float(loss)`` syncs become ONE device->host copy after the replay.  It is captured by
driving the engine directly on the capturing thread (forward, fused loss kernels, backward, optimizer): no autograd
takes part, so an autograd graph that an earlier eager step left alive plays no role in the capture.

With ``distributed`` set (one process per GPU) the step is a CHAIN of graph segments cut at the gradient-bucket
boundaries of backward (head + upper decoder / deep decoder / deep encoder / rest, ``parallel.DEFAULT_BUCKET_BYTES``):
segment k ends by flattening bucket k into a static buffer; its all-reduce (RCCL through the C ABI, never captured) is
launched on a side stream behind an event and runs UNDER segment k+1; the last segment is the fused optimizer step,
which waits for every bucket.  Only the last, smallest bucket's collective is exposed.  Without it the same step body
is one graph: the chain without bucket boundaries.

Train controls: with an ``optim.Adam(device_lr=True)`` (or ``optim.SGD`` / ``optim.RMSprop``) every call
uploads a changed ``group["lr"]`` before the replay, so host schedulers and manual edits take effect; ``scheduler=``
(``lr_scheduler.ReduceLROnPlateau``) is stepped with the total loss INSIDE the captured step, right behind the optimizer:
the reference's per-batch ``scheduler.step(pt_loss)`` without its host sync.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .engine import _tensor_dict, check_input
from .losses import LossSpec, _check_map, _total, select_loss_terms
from .parallel import DEFAULT_BUCKET_BYTES, get_communicator, make_sync


class _Segmenter:
    """The ``sync`` object ``UNetEngine.backward`` pushes gradients into: collects them into buckets and calls
    ``boundary(flat)`` whenever one is complete (and once more from ``finish``)."""

    def __init__(self, bucket_bytes: int, boundary):
        self.bucket_bytes, self.boundary = int(bucket_bytes), boundary
        self.pending: List[Tuple[str, torch.Tensor]] = []
        self.nbytes = 0
        self.layout: List[List[Tuple[str, torch.Size, int]]] = []
        self.flats: List[torch.Tensor] = []

    def _close(self) -> None:
        if not self.pending:
            return
        flat = torch.cat([g.reshape(-1) for _, g in self.pending])
        lay, off = [], 0
        for name, g in self.pending:
            lay.append((name, g.shape, off))
            off += g.numel()
        self.layout.append(lay)
        self.flats.append(flat)
        self.pending, self.nbytes = [], 0
        self.boundary(len(self.flats) - 1, flat)

    def push(self, named_grads) -> None:
        for name, g in named_grads:
            self.pending.append((name, g))
            self.nbytes += g.numel() * g.element_size()
        if self.nbytes >= self.bucket_bytes:
            self._close()

    def finish(self) -> Dict[str, torch.Tensor]:
        self._close()
        out = {}
        for flat, lay in zip(self.flats, self.layout):
            for name, shape, off in lay:
                out[name] = flat[off:off + shape.numel()].view(shape)
        return out


class GraphedTrainStep:
    """model: a ctunet_amd model on the GPU; optimizer: ctunet_amd.optim.Adam/AdamW/SGD/RMSprop (or torch.optim with
    capturable=True).
    ``loss``: a ``losses.LossSpec`` in place of the two lambdas (class weights, focal, Tversky and boundary terms); with a
    boundary term ``example_boundary`` holds one signed distance map per target and ``self.boundary`` the static copies the
    replay reads.
    ``x.grad`` is not filled: the input gradient kernels run (``input_requires_grad``), their result is not kept."""

    def __init__(self, model: torch.nn.Module, optimizer: torch.optim.Optimizer, example_input: torch.Tensor,
                 example_targets: Sequence[torch.Tensor], ce_lambda: float, dice_lambda: float,
                 input_requires_grad: bool = True, warmup: int = 3, distributed: bool = False, process_group=None,
                 bucket_bytes: Optional[int] = None, scheduler=None, loss: Optional[LossSpec] = None,
                 example_boundary: Optional[Sequence[torch.Tensor]] = None):
        self.model, self.opt = model, optimizer
        self.scheduler = scheduler
        if scheduler is not None and getattr(scheduler, "optimizer", optimizer) is not optimizer:
            raise ValueError("GraphedTrainStep: the scheduler belongs to another optimizer")
        # distributed + scheduler: the ranks' mean total loss, so that every rank takes the same decision (one float)
        self._metric = torch.zeros(1, dtype=torch.float32, device=example_input.device) \
            if scheduler is not None and distributed else None
        if loss is not None:                   # overrides the two lambdas
            if not any(loss.lambdas):
                raise ValueError("GraphedTrainStep: every lambda of the LossSpec is 0: there is no loss to train on")
            ce_lambda, dice_lambda = loss.ce_lambda, loss.dice_lambda
        self.ce, self.dice = float(ce_lambda), float(dice_lambda)
        if loss is None and not self.ce and not self.dice:
            raise ValueError("GraphedTrainStep: ce_lambda and dice_lambda are both 0: there is no loss to train on")
        self.spec = loss if loss is not None else LossSpec(self.ce, self.dice)
        n_maps = -1 if example_boundary is None else len(example_boundary)
        if self.spec.boundary_lambda != 0 and n_maps != len(example_targets):
            raise ValueError("GraphedTrainStep: boundary_lambda != 0 needs example_boundary, one signed distance map per "
                             "target (losses.boundary_map)")
        scaler = getattr(model, "loss_scaler", None)
        if scaler is not None and not hasattr(optimizer, "guard"):
            raise RuntimeError("GraphedTrainStep: a model with dynamic loss scaling needs an optimizer that reads the device "
                               "overflow flag (ctunet_amd.optim.Adam / AdamW / SGD / RMSprop); loss_scaler.step(optimizer) "
                               "would need a host sync inside the captured step")
        if hasattr(optimizer, "guard"):
            optimizer.guard(model)             # fp16: an overflowed step is skipped inside the replayed graph too
        if scaler is not None:                 # (dynamic: its state must exist on the GPU before anything is captured)
            scaler.prepare(example_input.device, example_input.shape[0] * example_input[0, 0].numel())
        self._params = [p for p in model.parameters()]
        self.distributed, self.group = distributed, process_group
        if distributed and model.__dict__.get("_grad_sync_cfg") is not None:
            raise RuntimeError("GraphedTrainStep(distributed=True) does its own all-reduce: do not also call "
                               "parallel.distribute() on the model (use parallel.broadcast_parameters)")
        self.x = example_input.detach().clone()
        self.targets = [t.detach().clone().contiguous() for t in example_targets]
        # the boundary term's signed distance maps: static buffers like the targets (``step.boundary[i].copy_(new_map)``)
        self.boundary: Optional[List[torch.Tensor]] = None
        if self.spec.boundary_lambda != 0:
            self.boundary = [b.detach().clone().contiguous() for b in example_boundary]
        self.x_req = input_requires_grad
        self.values: Optional[torch.Tensor] = None
        self.keys: List[str] = []              # set by _step
        self.skip_comm = False                 # measurement only (bench.py's comm_ms_exposed): replay without the collectives
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        if not distributed:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    self._step(make_sync(model))
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            with ops.gc_paused(), torch.cuda.graph(self.graph):
                self.values = self._step(make_sync(model))
            return
        import torch.distributed as dist
        self.world = dist.get_world_size(process_group)
        self.bucket_bytes = DEFAULT_BUCKET_BYTES if bucket_bytes is None else int(bucket_bytes)
        self.comm = get_communicator(process_group)
        self.comm_stream = torch.cuda.Stream()
        self.segments: List[torch.cuda.CUDAGraph] = []
        self.flats: List[torch.Tensor] = []
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):            # (the optimizer state must exist before its segment is captured)
                self._step(_Segmenter(self.bucket_bytes, self._allreduce_now))
            torch.cuda.synchronize()
            # with a process group alive other threads of the process may issue HIP calls while this one captures (the
            # nccl backend's watchdog polls its events): thread-local capture mode, see DESIGN 6
            self._capture_segments()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def _step(self, sync) -> torch.Tensor:
        """One train step, the engine driven directly: forward, the fused loss kernels (each head's gradient seeded with
        1, as autograd seeds it), backward pushing the gradients into ``sync``, optimizer.  Returns the loss terms and
        their sum, order ``keys``.  The input / target checks of the eager path are host-side only."""
        model = self.model
        check_input(model, self.x)
        eng = model._engine()
        P = _tensor_dict(model)
        with torch.no_grad():
            out0, out1, ctx = eng.forward(P, self.x, model.training, True, bool(getattr(model, "chk", False)))
            outs = [out0] if out1 is None else [out0, out1]
            if len(outs) != len(self.targets):
                raise RuntimeError(f"GraphedTrainStep: {len(self.targets)} target(s) for {len(outs)} model output(s)")
            two = out1 is not None
            heads, gouts = [], []
            spec = self.spec
            for i, (o, t) in enumerate(zip(outs, self.targets)):
                _check_map(o, t)
                if spec.extended:
                    phi = None if self.boundary is None else self.boundary[i]
                    terms, ws = ops.seg_loss_fwd(o, t, spec.lambdas, two, boundary=phi, **spec.kernel_args)
                    gouts.append(ops.seg_loss_bwd(o, t, spec.lambdas, two, ws, boundary=phi, **spec.kernel_args))
                    heads.append((terms[0], terms[1], terms[2], terms[3]))
                else:
                    terms, ws = ops.loss_fwd(o, t, self.ce, self.dice, two)
                    gouts.append(ops.loss_bwd(o, t, self.ce, self.dice, two, ws, None, None))
                    heads.append((terms[0], terms[1], None, None))
            keys, tl = select_loss_terms(heads, spec)
            values = torch.stack(tl + [_total(tl)])
            if self._metric is not None:
                self._metric.copy_(values[-1:])            # (before backward: in the first segment of the chain)
                if not torch.cuda.is_current_stream_capturing():
                    self._allreduce_now(-1, self._metric)  # warm-up; replays launch it from __call__, never captured
            grads, _ = eng.backward(P, ctx, gouts[0], gouts[1] if two else None, self.x_req, sync)
            for name, p in model.named_parameters():
                p.grad = grads.get(name) if p.requires_grad else None
            self.opt.step()
            if self.scheduler is not None:
                self.scheduler.step(values[-1] if self._metric is None else self._metric)
            for p in self._params:
                p.grad = None
        self.keys = keys + ["epoch_loss"]
        return values

    # ------------------------------------------------------------------ segmented (N > 1)
    def _allreduce_now(self, k: int, flat: torch.Tensor) -> None:
        """Bucket boundary of a warm-up step: the all-reduce, waited for at once (not timed; finish() then hands back
        reduced gradients, as GradSync's does)."""
        self._launch_allreduce(flat)
        torch.cuda.current_stream().wait_stream(self.comm_stream)

    def _capture_segments(self) -> None:
        """Captures the step as a chain: every bucket boundary ends the segment being captured and begins the next one
        in the same memory pool; the overflow fold and the optimizer step end up in the last segment."""
        def begin():
            g = torch.cuda.CUDAGraph()
            g.capture_begin(pool=self.segments[0].pool() if self.segments else None, capture_error_mode="thread_local")
            self.segments.append(g)

        def boundary(k: int, flat: torch.Tensor) -> None:
            self.flats.append(flat)
            self.segments[-1].capture_end()
            begin()

        with ops.gc_paused():
            begin()
            self.values = self._step(_Segmenter(self.bucket_bytes, boundary))
            self.segments[-1].capture_end()

    def _launch_allreduce(self, flat: torch.Tensor) -> None:
        """Mean over ranks of one bucket on the side stream, behind everything enqueued on the current stream so far."""
        cur = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(cur)
        self.comm_stream.wait_event(ev)
        self.comm.allreduce_(flat, average=True, stream=self.comm_stream)

    def __call__(self, x: Optional[torch.Tensor] = None, targets: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
        """Copies the batch into the captured buffers, replays the step, returns the loss terms (device tensor,
        order ``self.keys``); call ``.tolist()`` on it for the reference's logged floats (one sync)."""
        if x is not None:
            self.x.detach().copy_(x)
        if targets is not None:
            for dst, src in zip(self.targets, targets):
                dst.copy_(src)
        if hasattr(self.opt, "sync_lr"):
            self.opt.sync_lr()                     # a host-side edit of group["lr"] reaches the replay (device_lr=True only)
        if not self.distributed:
            self.graph.replay()
        else:
            cur = torch.cuda.current_stream()
            for k, flat in enumerate(self.flats):
                self.segments[k].replay()
                if not self.skip_comm:
                    self._launch_allreduce(flat)           # runs under segment k + 1
                    if k == 0 and self._metric is not None:
                        self._launch_allreduce(self._metric)        # 4 bytes, under the rest of backward
            cur.wait_stream(self.comm_stream)
            self.segments[-1].replay()                    # the fused optimizer step, reading the averaged buckets
        # the replayed optimizer kernel wrote the parameters through raw pointers: bump their version counters, so that
        # an eagerly launched forward after this replay (the reference's train-then-validate epoch loop,
        # Model.py:240-243) re-packs the engine's MFMA-ordered weight copies instead of hitting a stale cache entry
        torch.autograd.graph.increment_version(self._params)
        return self.values
