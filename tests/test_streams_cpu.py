"""titok_video_amd/streams.py, the cross-stream ownership rule, driven with stub streams that record who was made to wait for what.
No torch device: the rule's logic is the caller-independent part (where the calls are placed is a race no timing test shows)."""
from titok_video_amd.streams import EventOnce, StreamOwned


class Stream:
    def __init__(self, sid, log):
        self.cuda_stream, self.log = sid, log

    def __eq__(self, other):
        return self.cuda_stream == other.cuda_stream

    __hash__ = None      # the rule keys streams by id, as for torch streams, never by hashing the stub

    def wait_event(self, event):
        self.log.append((self.cuda_stream, "event", event))

    def wait_stream(self, other):
        self.log.append((self.cuda_stream, "stream", other.cuda_stream))


def _owned():
    log = []
    build, a, b, c = (Stream(i, log) for i in (10, 11, 12, 13))
    return log, StreamOwned(build, "ready"), build, a, b, c


def test_build_stream_never_waits_on_use_and_foreign_streams_wait_once():
    log, owned, build, a, b, _c = _owned()
    for _ in range(3):
        owned.use(build)
    assert log == []
    for _ in range(3):
        owned.use(a)
        owned.use(Stream(11, log))      # the same stream through another handle
        owned.use(b)
        owned.use(build)
    assert log == [(11, "event", "ready"), (12, "event", "ready")]


def test_retire_from_the_build_stream_waits_for_every_other_reader_only():
    log, owned, build, a, b, c = _owned()
    for st in (build, a, b, a):
        owned.use(st)
    del log[:]
    owned.retire(build)
    assert sorted(log) == [(10, "stream", 11), (10, "stream", 12)]      # not for itself, not for c (never a reader), nobody else waits
    # a plan that only its build stream ever used: nothing to wait for
    log2, alone, build2, *_ = _owned()
    alone.use(build2)
    alone.retire(build2)
    assert log2 == []


def test_retire_from_a_foreign_stream_makes_it_and_the_build_stream_wait():
    log, owned, build, a, b, c = _owned()
    for st in (build, a, b, c):
        owned.use(st)
    del log[:]
    owned.retire(c)
    waits_c = sorted(w for w in log if w[0] == 13)
    waits_build = sorted(w for w in log if w[0] == 10)
    assert waits_c == [(13, "stream", 10), (13, "stream", 11), (13, "stream", 12)]       # every reader but itself
    # the build stream: every reader other than itself and c - and c, which read the object too: the memory returns to the build
    # stream's pool, which has to see c's reads finished like anybody's (the rule as BatchPlan.retire / _retire_pack always had it)
    assert waits_build == [(10, "stream", 11), (10, "stream", 12), (10, "stream", 13)]
    assert len(log) == 6                                                                    # and nobody else waits
    # released by a stream that never read it, the build stream not among the readers either
    log, owned, build, a, b, c = _owned()
    owned.use(a)
    del log[:]
    owned.retire(b)
    assert sorted(log) == [(10, "stream", 11), (12, "stream", 11)]


def test_one_event_form_waits_once_per_foreign_stream_and_never_on_the_build_stream():
    log = []
    build, a, b = (Stream(i, log) for i in (10, 11, 12))
    done = EventOnce(build, "done")
    for _ in range(3):
        done.wait_once(build)
        done.wait_once(a)
        done.wait_once(b)
        done.wait_once(Stream(12, log))
    assert log == [(11, "event", "done"), (12, "event", "done")]
