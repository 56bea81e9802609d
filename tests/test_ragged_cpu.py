"""Ragged decoding, host-side pieces (no GPU): the C ABI's new entries and the slot scheduler of Engine.generate_stream driven by a stub
step function."""
import ctypes
import random

import pytest

ENTRIES = ("coati_attn_decode_rows", "coati_topk_sample_rows", "coati_engine_decode_step_rows", "coati_engine_decode_prefill_rows")


def test_header_declares_and_library_exports_ragged_entries():
    from coati_amd import _lib
    l = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and _lib.PROTOTYPES[name][0] is ctypes.c_int, name
        assert hasattr(l, name), name
        assert name in _lib.exported_symbols()


def _simulate(lengths, slots):
    """Direct simulation of a greedy refill: before every step the free slots take the queue's next requests, then every busy slot
    emits one token; request n leaves its slot with its lengths[n]-th token.  Returns the number of steps."""
    left = [0] * slots          # tokens the slot's request still has to emit (0 = free)
    nxt, steps = 0, 0
    while nxt < len(lengths) or any(left):
        for s in range(slots):
            if left[s] == 0 and nxt < len(lengths):
                left[s] = lengths[nxt]
                nxt += 1
        left = [max(0, x - 1) for x in left]
        steps += 1
    return steps


def _drive(lengths, slots, poll=1):
    from coati_amd.slots import SlotScheduler
    sched = SlotScheduler(len(lengths), slots)
    emitted = {}                 # slot -> [request, tokens so far]
    served = []

    def step(new):
        for s, r in new:
            assert s not in emitted, "a busy slot was refilled"
            emitted[s] = [r, []]
            served.append(r)
        ended = []
        for s in sorted(emitted):
            r, toks = emitted[s]
            toks.append((r, len(toks)))
            if len(toks) == lengths[r]:
                ended.append((s, toks))
        for s, _ in ended:
            del emitted[s]
        return ended

    rows, steps = sched.run(step, poll=poll)
    assert sched.finished and sched.live == 0 and not emitted
    return rows, steps, served


CASES = [
    ([5], 1), ([3, 1, 4, 1, 5, 9, 2, 6], 1), ([3, 1, 4, 1, 5, 9, 2, 6], 3), ([7, 7, 7, 7], 4), ([2, 9], 8),
    ([1] * 13, 4), ([38 + (7 * i) % 39 for i in range(100)], 16), ([1 + (i * i) % 50 for i in range(257)], 32),
]


@pytest.mark.parametrize("lengths,slots", CASES)
def test_scheduler_serves_every_request_once_in_order_and_greedily(lengths, slots):
    from coati_amd.slots import greedy_steps
    rows, steps, served = _drive(lengths, slots)
    assert served == list(range(len(lengths)))                       # requests enter in order, each once
    assert len(rows) == len(lengths)
    for n, row in enumerate(rows):                                     # results in request order, each the request's own tokens
        assert row == [(n, i) for i in range(lengths[n])], n
    assert steps == _simulate(lengths, slots) == greedy_steps(lengths, slots)


def test_scheduler_random_sets_and_polling():
    rng = random.Random(5)
    for _ in range(40):
        n, slots = rng.randint(1, 60), rng.randint(1, 12)
        lengths = [rng.randint(1, 20) for _ in range(n)]
        rows, steps, served = _drive(lengths, slots)
        assert served == list(range(n)) and [len(r) for r in rows] == lengths
        assert steps == _simulate(lengths, slots)
        # looking for free slots every 4th step only: still every request once and in order, never fewer steps than greedy
        rows4, steps4, served4 = _drive(lengths, slots, poll=4)
        assert served4 == served and rows4 == rows and steps4 >= steps


def test_scheduler_refusals():
    from coati_amd.slots import SlotScheduler
    with pytest.raises(ValueError):
        SlotScheduler(4, 0)
    s = SlotScheduler(2, 4)
    assert s.refill() == [(0, 0), (1, 1)] and s.live == 2 and s.refill() == []
    with pytest.raises(ValueError):
        s.retire(3)
    assert s.retire(1) == 1 and s.retire(0) == 0 and s.finished
