"""Host staging, once for every pipeline: which models take the device path (``device_path``) and how host data reaches the
engine's GPU -- uint8 frames through the process-wide ``pinned_pool`` (``upload``, ``wait_upload``), small tables through
``upload_table`` -- and how a model that takes a host path is called (``call_host``).  ``StreamBatcher``'s window buffers are NOT in the pool: they are filled when a frame arrives, long before the
copy, and have a byte budget of their own."""
from __future__ import annotations

import threading
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch


def engine_device(model) -> Optional[torch.device]:
    if hasattr(model, 'forward_device') and torch.cuda.is_available():
        return torch.device('cuda', getattr(model, 'device', 0))
    return None


def device_path(model) -> bool:
    """``model`` is a ``TsmEngine`` on a GPU: frames are staged to its device and transformed by the HIP kernels straight
    into its packed input.  Anything else (a session, a stub, a torch module, no GPU) takes a host path."""
    return engine_device(model) is not None and hasattr(model, 'packed_layout')


class PinnedPool:
    """Reusable page-locked staging buffers.  Pinning fresh memory for every video costs a hipHostMalloc /
    hipHostFree pair that serialises with the GPU queue; here a few flat byte buffers are grown geometrically
    and handed out round-robin.  Ownership is explicit: ``take`` hands a slot to exactly one user (the prefetch
    worker thread and the main thread's oversized-video loop share the pool) and the slot stays taken -- while it
    is being filled on the host AND while the H2D copy out of it is in flight -- until that user calls ``release``
    with the event recorded behind its copy; the next taker of the slot waits for the release, then for the event.
    ``alloc(nbytes) -> uint8 [nbytes]`` makes the buffers (default: page-locked; a test without a GPU passes pageable)."""

    def __init__(self, slots: int = 3, alloc: Optional[Callable[[int], torch.Tensor]] = None):
        self.alloc = alloc or (lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, pin_memory=True))
        self.bufs: List[Optional[torch.Tensor]] = [None] * slots
        self.busy: List[Optional[object]] = [None] * slots      # event of the last copy out of the slot
        self.taken: List[bool] = [False] * slots                # handed out and not yet released
        self.next = 0
        self.cv = threading.Condition()

    def take(self, nbytes: int) -> Tuple[torch.Tensor, int]:
        with self.cv:
            i = self.next
            self.next = (i + 1) % len(self.bufs)
            while self.taken[i]:
                self.cv.wait()
            self.taken[i] = True
            ev, self.busy[i] = self.busy[i], None
        try:
            if ev is not None:
                ev.synchronize()
            if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
                self.bufs[i] = None                              # free before growing
                self.bufs[i] = self.alloc(max(nbytes, 1 << 20) * 5 // 4)
        except BaseException:
            # (a failed event wait or pinned allocation: upload's try/finally only starts once take() has returned,
            #  so the slot is handed back here -- the next taker must get an error or a buffer, never an endless wait)
            self.release(i, None)
            raise
        return self.bufs[i][:nbytes], i

    def release(self, slot: int, event: Optional[object]) -> None:
        """The user's host fill is done and its H2D copy is enqueued; ``event`` completes when the copy has."""
        with self.cv:
            self.busy[slot] = event
            self.taken[slot] = False
            self.cv.notify_all()


pinned_pool = PinnedPool()


def upload(shape: Sequence[int], fill: Callable[[torch.Tensor], None], dev: torch.device, stream: Optional[object] = None,
           pool: PinnedPool = pinned_pool) -> Tuple[torch.Tensor, object]:
    """uint8 ``shape`` to ``dev`` through a pool slot: ``fill(pinned view)`` writes it on the host, the copy is enqueued on
    ``stream`` (default: the device's current one; a side stream lets the copy of video i+1 run under the compute of video
    i) and the event recorded behind it on that stream goes to the pool with the slot.  Returns (device tensor, event).  The
    slot is held across fill and copy; a ``fill`` that raises gives it back with no event and the exception propagates."""
    flat, slot = pool.take(int(np.prod(shape)))
    ready = None
    try:
        pinned = flat.view(tuple(shape))
        fill(pinned)
        with torch.cuda.stream(stream):                  # (a no-op context for None)
            out = pinned.to(dev, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(dev))
    finally:
        pool.release(slot, ready)
    return out, ready


def wait_upload(frames: torch.Tensor, ready) -> None:
    """The consumer half of an ``upload`` on another stream: the device's current stream waits for the copy, and the caching
    allocator learns that this stream uses the block too (it was allocated on the copy's stream)."""
    cur = torch.cuda.current_stream(frames.device)
    cur.wait_event(ready)
    frames.record_stream(cur)


def upload_table(host: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """A small host tensor (boxes, an index table, counters) to ``dev`` without blocking."""
    # (page-locked staging from torch's caching host allocator: an upload from pageable memory would wait for the
    #  batches already queued on the stream)
    staged = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
    staged.copy_(host)
    return staged.to(dev, non_blocking=True)


def call_host(model, x: torch.Tensor, one_per_run: bool = False) -> np.ndarray:
    """A model without a device path on a batch ``x`` -> float32 ndarray: the one way the pipelines call it.  The onnxruntime
    duck type (``run`` + ``get_inputs``) gets ``run(None, {first input name: x as numpy})[0]`` -- with ``one_per_run`` one ``run``
    per row of ``x``, as the reference feeds the image model; anything else is ``call_host_module``'s."""
    if not (hasattr(model, 'run') and hasattr(model, 'get_inputs')):
        return call_host_module(model, x)
    name, feed = model.get_inputs()[0].name, x.cpu().numpy()
    if one_per_run:
        return np.concatenate([np.asarray(model.run(None, {name: feed[i:i + 1]})[0], dtype=np.float32) for i in range(len(feed))])
    return np.asarray(model.run(None, {name: feed})[0], dtype=np.float32)


def call_host_module(model, x: torch.Tensor) -> np.ndarray:
    """``model(x)`` for a torch module (``x`` goes to the device of its parameters first) or any callable -> float32 ndarray."""
    with torch.no_grad():
        p = next(iter(model.parameters()), None) if hasattr(model, 'parameters') else None
        y = model(x.to(p.device) if p is not None else x)
    return np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y, dtype=np.float32)
