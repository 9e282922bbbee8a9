"""The staging contract without a GPU: ``staging.PinnedPool`` driven through its injected allocator (pageable memory) with
fake events that log ``synchronize()``, and the piece arithmetic of ``inference_count`` against brute force.  Every step that
may block runs in a thread joined with a timeout, so a broken pool fails a test instead of hanging the suite."""
import threading

import pytest
import torch

from workoutdetector_amd import inference_count as ic
from workoutdetector_amd.staging import PinnedPool

JOIN = 10.0          # seconds a thread may take where it must not block at all


class FakeEvent:
    def __init__(self, log, name, error=None):
        self.log, self.name, self.error = log, name, error

    def synchronize(self):
        self.log.append(self.name)
        if self.error is not None:
            raise self.error


def pageable(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8)


def take_in_thread(pool, nbytes):
    """Start ``pool.take(nbytes)`` on a thread -> (thread, box); box['got'] = (view, slot) or box['error'] once it returned."""
    box = {}

    def run():
        try:
            box['got'] = pool.take(nbytes)
        except BaseException as exc:
            box['error'] = exc
    t = threading.Thread(target=run, daemon=True)
    t.start()
    return t, box


def take_now(pool, nbytes):
    t, box = take_in_thread(pool, nbytes)
    t.join(JOIN)
    assert not t.is_alive(), 'take() blocked on a free slot'
    if 'error' in box:
        raise box['error']
    return box['got']


def test_a_third_take_waits_for_the_release_and_then_for_its_event():
    log = []
    pool = PinnedPool(slots=2, alloc=pageable)
    (_, s0), (_, s1) = take_now(pool, 100), take_now(pool, 100)
    assert (s0, s1) == (0, 1) and pool.taken == [True, True]
    waits, cv_wait = threading.Semaphore(0), pool.cv.wait
    pool.cv.wait = lambda timeout=None: (waits.release(), cv_wait(timeout))[1]      # tells the test that take() is waiting
    t, box = take_in_thread(pool, 100)                  # round-robin: slot 0 again, still taken
    assert waits.acquire(timeout=JOIN) and t.is_alive() and not box and log == []
    pool.release(s1, FakeEvent(log, 'copy1'))           # not the slot it waits for: woken, it waits again
    assert waits.acquire(timeout=JOIN) and t.is_alive() and not box and log == []
    pool.release(s0, FakeEvent(log, 'copy0'))
    t.join(JOIN)
    assert not t.is_alive() and box['got'][1] == 0
    assert log == ['copy0']                             # synchronised before take() returned; slot 1's event untouched
    assert pool.taken == [True, False] and pool.busy[0] is None


def test_a_larger_request_replaces_the_buffer_and_a_smaller_one_reuses_it():
    sizes = []

    def alloc(nbytes):
        sizes.append(nbytes)
        return pageable(nbytes)
    pool = PinnedPool(slots=1, alloc=alloc)
    view, slot = take_now(pool, 3 << 20)
    assert view.numel() == 3 << 20 and view.dtype == torch.uint8 and sizes == [(3 << 20) * 5 // 4]
    first = view.data_ptr()
    pool.release(slot, None)
    view, slot = take_now(pool, 1000)                   # smaller: the same storage
    assert view.numel() == 1000 and view.data_ptr() == first and len(sizes) == 1
    pool.release(slot, None)
    view, slot = take_now(pool, (3 << 20) * 5 // 4)     # exactly the buffer: still no new one
    assert view.data_ptr() == first and len(sizes) == 1
    pool.release(slot, None)
    view, slot = take_now(pool, 4 << 20)                # larger: replaced, grown by a quarter
    assert view.numel() == 4 << 20 and sizes == [(3 << 20) * 5 // 4, (4 << 20) * 5 // 4]
    assert pool.bufs[0].numel() == sizes[-1]
    pool.release(slot, None)
    assert take_now(PinnedPool(slots=1, alloc=alloc), 10)[0].numel() == 10 and sizes[-1] == (1 << 20) * 5 // 4   # the floor


def test_a_failing_allocator_or_event_propagates_and_frees_the_slot():
    log, fail = [], [MemoryError('no page-locked memory')]

    def alloc(nbytes):
        if fail:
            raise fail.pop()
        return pageable(nbytes)
    pool = PinnedPool(slots=1, alloc=alloc)
    with pytest.raises(MemoryError, match='no page-locked memory'):
        take_now(pool, 100)
    assert pool.taken == [False] and pool.busy == [None]
    view, slot = take_now(pool, 100)                    # the same slot, without waiting
    assert slot == 0 and view.numel() == 100
    pool.release(slot, FakeEvent(log, 'lost', RuntimeError('device lost')))
    with pytest.raises(RuntimeError, match='device lost'):
        take_now(pool, 100)
    assert log == ['lost'] and pool.taken == [False] and pool.busy == [None]
    assert take_now(pool, 100)[1] == 0 and log == ['lost']       # the failed event is gone: no second synchronise


def test_release_without_an_event_means_no_synchronise():
    log = []
    pool = PinnedPool(slots=1, alloc=pageable)
    _, slot = take_now(pool, 64)
    pool.release(slot, FakeEvent(log, 'copy'))
    _, slot = take_now(pool, 64)
    assert log == ['copy']
    pool.release(slot, None)
    assert take_now(pool, 64)[1] == 0 and log == ['copy']


# ---- piece arithmetic ---------------------------------------------------------------------------------------------------------
def test_even_frame_range_is_exactly_what_the_clips_sample():
    """For every video length 1..129 and every clip range [a, b): min .. max + 1 of the even-frame indices the clips' segments
    read (segment k of clip c reads source frame 8c + 2k when that is inside the video)."""
    for total in range(1, 130):
        n = len(ic.clip_starts(total))
        sampled = [[(8 * c + 2 * k) // 2 for k in range(8) if 8 * c + 2 * k < total] for c in range(n)]
        assert all(sampled)
        for a in range(n):
            for b in range(a + 1, n + 1):
                idx = [i for row in sampled[a:b] for i in row]
                assert ic.even_frame_range(total, a, b) == (min(idx), max(idx) + 1), (total, a, b)


def test_a_piece_of_clips_per_piece_clips_fits_the_budget(monkeypatch):
    """n clips stage 4 n + 4 even frames and the zero frame: whenever ``clips_per_piece`` is not clamped to its floor of 1
    that fits the budget, ``MAX_STAGE_BYTES`` as it is when the call is made; the floor is 1 whatever the sizes."""
    for per_frame in (1, 3, 90 * 52 * 3, 1080 * 1920 * 3):
        for budget in sorted({0, 1, per_frame, 9 * per_frame, 13 * per_frame - 1, 13 * per_frame, 16 * per_frame,
                              17 * per_frame - 1, 17 * per_frame, 40 * per_frame, 1000 * per_frame + 7, 1 << 30}):
            monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', budget)
            n = ic.clips_per_piece(per_frame)
            assert n >= 1
            if n > 1 or budget // per_frame >= 12:      # (not the floor: one clip's 8 even frames + 4 to the next clip fit)
                assert (4 * n + 5) * per_frame <= budget, (per_frame, budget, n)
    monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 100)
    assert ic.clips_per_piece(0) == 23                  # (a frame of no bytes counts as one byte)
    monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 40 * 90 * 52 * 3)
    assert ic.clips_per_piece(90 * 52 * 3) == 8
    monkeypatch.setattr(ic, 'MAX_STAGE_BYTES', 12 * 90 * 52 * 3)
    assert ic.clips_per_piece(90 * 52 * 3) == 1
