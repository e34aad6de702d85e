"""Tools of tests/test_gpu_streams.py: a delay that holds a stream, and a control read that
proves the delay was still holding it when the call under test was made.

A test queues ``delay()`` on a stream, then the producer work (a copy into a buffer the call
under test reads), then asks ``Control.check()``: device-to-host copies of that buffer on
fresh non-blocking streams, with no wait.  They must still see the old contents; if one sees
the new ones the window was not open and the test fails, because it would assert nothing.
"""
import functools
import time

import torch

TARGET_S = 0.2            # a delay lasts about this long: 0.1-0.3 s is accepted, never 0.5 s


def _timed(queue):
    """seconds the work ``queue()`` puts on the current stream takes, by two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    queue()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3


@functools.lru_cache(maxsize=None)
def _calibrated():
    """(queue, seconds): ``queue()`` puts a delay of ``seconds`` (0.1 to 0.3) on the current
    stream.  torch.cuda._sleep where the build has it (one tiny spinning kernel; its cycle
    unit is no clock here, so it is timed), else a chain of fp64 matmuls timed the same way."""
    if hasattr(torch.cuda, "_sleep"):
        unit = lambda n: torch.cuda._sleep(int(n))                       # noqa: E731
        n = 1 << 20
    else:
        a = torch.rand((1024, 1024), dtype=torch.float64, device="cuda")

        def unit(n):
            for _ in range(int(n)):
                torch.mm(a, a)
        n = 1
    unit(n)                                                  # first launch: module load
    t = _timed(lambda: unit(n))
    while t < 0.01 and n < (1 << 40):                        # long enough to time, far below 0.1 s
        n *= 4
        t = _timed(lambda: unit(n))
    for _ in range(2):                                       # scale to the target, then confirm
        n = max(1, int(n * TARGET_S / t))
        t = _timed(lambda: unit(n))
        if 0.1 <= t <= 0.3:
            break
    assert 0.1 <= t <= 0.3, f"could not calibrate a 0.1-0.3 s delay: {n} units take {t:.3f} s"
    return (lambda: unit(n)), t


def delay():
    """Queue the calibrated delay on the current stream."""
    _calibrated()[0]()


def delay_seconds():
    return _calibrated()[1]


class Control:
    """The control read of one device buffer.  Built before the delay is queued, with the
    device quiet: it keeps the buffer's old contents, page-locked landing buffers (allocating
    one later could wait for the device) and non-blocking streams of its own.

    Several streams, because a process's streams share a few hardware queues (4 by default)
    and two streams on one queue run in order: a control stream that shares the held stream's
    queue waits behind the delay like the producer does, and would then report the produced
    contents.  So the read is queued on every control stream without waiting, and the ones
    that complete at once are the control; the others are still held and say nothing."""

    WAYS = 8
    WAIT_S = 0.05             # a 100 KB copy takes microseconds; the delay lasts 0.1 s or more

    def __init__(self, buf):
        torch.cuda.synchronize()
        self.buf = buf
        self.old = buf.detach().cpu().clone()
        self.hosts = [torch.empty(buf.shape, dtype=buf.dtype, pin_memory=True)
                      for _ in range(self.WAYS)]
        self.streams = [torch.cuda.Stream() for _ in range(self.WAYS)]

    def check(self):
        """Called right after the producer work is queued behind the delay: the buffer, read
        on the control's own streams with no wait, still holds the old contents."""
        events = []
        for s, host in zip(self.streams, self.hosts):
            with torch.cuda.stream(s):
                host.copy_(self.buf, non_blocking=True)
                events.append(torch.cuda.Event())
                events[-1].record()
        done, t_end = [], time.perf_counter() + self.WAIT_S
        while not done and time.perf_counter() < t_end:
            done = [k for k, e in enumerate(events) if e.query()]
        assert done, ("no control read completed: every control stream waits behind the held "
                      "stream, so this test would assert nothing")
        for k in done:
            assert torch.equal(self.hosts[k], self.old), (
                "the delay did not hold: the control read already sees the produced contents, "
                "so this test would assert nothing")
