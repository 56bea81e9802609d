"""Slot bookkeeping of streamed generation (Engine.generate_stream): N requests share S cache slots; a slot whose row has ended is
handed the next request while the other rows carry on.  Plain host code, no device and no torch: the decode loop asks `refill()`
which requests enter which slots, runs its steps, and reports the slots whose rows ended with `retire()`.  `run()` drives a step
function through the whole queue (the engine's loop has the same shape; tests drive a stub with it)."""
from typing import Callable, Dict, Iterable, List, Sequence, Tuple

STREAM_SLOT_CAP = 1024   # default slot count of generate_stream: the batch at which the decode step stops being launch-bound
#                          (1.2 ms per step against 0.7 ms at 64 rows) and the KV cache of the grande shape is ~ 4 GB


class SlotScheduler:
    """Requests 0 .. n_requests - 1 enter the slots in order; each is served by exactly one slot, once."""

    def __init__(self, n_requests: int, slots: int):
        if n_requests < 0 or slots < 1:
            raise ValueError(f"SlotScheduler: {n_requests} requests on {slots} slots")
        self.n_requests = int(n_requests)
        self.slots = int(slots)
        self.slot_req: List[int] = [-1] * self.slots   # request a slot serves, -1 = free
        self.next_request = 0
        self.n_retired = 0
        self._free: List[int] = list(range(self.slots))   # ascending: the lowest free slot is filled first

    def refill(self) -> List[Tuple[int, int]]:
        """Hand the queue's next requests to the free slots: [(slot, request)], possibly empty."""
        got = []
        while self._free and self.next_request < self.n_requests:
            s = self._free.pop(0)
            self.slot_req[s] = self.next_request
            got.append((s, self.next_request))
            self.next_request += 1
        return got

    def retire(self, slot: int) -> int:
        """The row in `slot` has ended: the slot is free again.  Returns the request it served."""
        r = self.slot_req[slot]
        if r < 0:
            raise ValueError(f"SlotScheduler: slot {slot} is not busy")
        self.slot_req[slot] = -1
        self._free.append(slot)
        self._free.sort()
        self.n_retired += 1
        return r

    @property
    def live(self) -> int:
        return self.slots - len(self._free)

    @property
    def finished(self) -> bool:
        return self.n_retired == self.n_requests

    def run(self, step: Callable[[Sequence[Tuple[int, int]]], Iterable[Tuple[int, object]]], poll: int = 1):
        """Drive `step` until every request has been served.  step(new) loads the (slot, request) pairs of `new`, advances every
        busy slot by ONE token and returns [(slot, result)] for the slots whose rows ended in that step.  The scheduler looks for
        free slots every `poll` steps (poll = 1: a freed slot is refilled before the very next step).  Returns (results in
        request order, number of steps)."""
        results: Dict[int, object] = {}
        steps = 0
        while not self.finished:
            new = self.refill()
            ended = []
            for i in range(max(1, int(poll))):
                ended += list(step(new if i == 0 else []))
                steps += 1
                if len(ended) == self.live:   # nothing left to advance
                    break
            for slot, res in ended:
                results[self.retire(slot)] = res
        return [results[n] for n in range(self.n_requests)], steps


def greedy_steps(lengths: Sequence[int], slots: int) -> int:
    """Steps a greedy refill takes when request n occupies a slot for lengths[n] steps: the makespan of list scheduling in request
    order on `slots` machines (the time the last slot falls idle)."""
    busy_until = [0] * max(1, int(slots))
    for n in lengths:
        i = busy_until.index(min(busy_until))
        busy_until[i] += int(n)
    return max(busy_until) if len(lengths) else 0
