"""Who may touch a device object that several streams share (ForwardPipeline): the ownership rule, stated once.

An object is built by work queued on one stream, the build stream, whose allocator pool owns its memory.  Any other stream waits
for the build's event before its first read.  Before the object is released, the releasing stream and the build stream wait for
every stream that read it: the memory returns to the build stream's pool, which could hand it out again while a reader is still
running.

Nothing here calls torch: the caller passes the current stream in.  A stream is anything with `wait_event`, `wait_stream`, `==`
and a `cuda_stream` id (torch.cuda.Stream; the stubs of tests/test_streams_cpu.py).  Host objects own no streams: their holders
keep None in place of one of these.
"""
from __future__ import annotations


class EventOnce:
    """Part of an owned object that was queued later on its build stream (an attention table of a plan, a decoder's constant block):
    one event, waited for once by every other stream.  The build stream is ordered behind it already and never waits."""

    def __init__(self, build_stream, event):
        self.build_stream, self.event = build_stream, event
        self._seen = set()

    def wait_once(self, cur) -> None:
        if cur != self.build_stream and cur.cuda_stream not in self._seen:
            cur.wait_event(self.event)
            self._seen.add(cur.cuda_stream)


class StreamOwned:
    """A device object built on `build_stream`, complete once `ready_event` has passed."""

    def __init__(self, build_stream, ready_event):
        self.build_stream, self.ready = build_stream, ready_event
        self._readers = {}      # stream id -> stream, the build stream included

    def use(self, cur) -> None:
        """Before `cur` reads the object: a foreign stream waits for the build on its first use; every user is remembered."""
        if cur != self.build_stream and cur.cuda_stream not in self._readers:
            cur.wait_event(self.ready)
        self._readers[cur.cuda_stream] = cur

    def retire(self, cur) -> None:
        """Before the object is released from `cur`: `cur` waits for every other reader, and so does the build stream when it is
        not `cur` itself (a release noticed on a pipeline's side stream frees into the build stream's pool)."""
        build = self.build_stream
        for st in self._readers.values():
            if st != cur:
                cur.wait_stream(st)
            if build != cur and st != build:
                build.wait_stream(st)
