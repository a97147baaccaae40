"""worker.DeviceScope against a fake worker, no library: what a scope frees and when, on every exit (tests/test_gpu_buffer_ownership.py drives
the real entry points through the same failures)."""
import numpy as np
import pytest

from distributed_plonk_amd.worker import DeviceScope, PlonkWorker, closing_on_error


class Boom(Exception):
    pass


class FakeBuffer:
    def __init__(self, worker, nbytes):
        self.worker, self.nbytes, self.ptr, self.frees = worker, nbytes, 0x1000 + len(worker.bufs), 0

    def upload(self, arr):
        if self.worker.fail_upload:
            raise Boom("upload")
        self.data = np.array(arr)
        return self

    def free(self):
        if self.ptr:
            if self in self.worker.fail_free:
                raise Boom(f"free {self.worker.bufs.index(self)}")
            self.ptr, self.frees = None, self.frees + 1


class FakeWorker:
    def __init__(self, fail_alloc_at=None):
        self.bufs, self.fail_alloc_at, self.fail_upload, self.fail_free = [], fail_alloc_at, False, []

    def alloc(self, nbytes):
        if len(self.bufs) == self.fail_alloc_at:
            raise Boom("alloc")
        self.bufs.append(FakeBuffer(self, nbytes))
        return self.bufs[-1]

    scope = PlonkWorker.scope

    def live(self):
        return sum(1 for b in self.bufs if b.ptr)


def test_exit_frees_everything_on_success_and_on_exception():
    w = FakeWorker()
    with w.scope() as s:
        assert isinstance(s, DeviceScope) and s.worker is w
        a, b = s.alloc(16), s.upload(np.arange(4, dtype=np.uint64))
        assert (a.nbytes, b.nbytes) == (16, 32) and np.array_equal(b.data, np.arange(4)) and w.live() == 2
    assert w.live() == 0 and [x.frees for x in w.bufs] == [1, 1]
    with pytest.raises(Boom, match="later"):
        with w.scope() as s:
            s.alloc(8), s.alloc(8)
            raise Boom("later")
    assert w.live() == 0 and len(w.bufs) == 4


def test_a_failing_upload_still_frees_its_buffer():
    w = FakeWorker()
    w.fail_upload = True
    with pytest.raises(Boom, match="upload"):
        with w.scope() as s:
            s.alloc(8)
            s.upload(np.zeros(3, dtype=np.uint8))
    assert len(w.bufs) == 2 and w.bufs[1].nbytes == 3 and w.live() == 0


def test_an_alloc_that_fails_midway_frees_the_earlier_buffers():
    w = FakeWorker(fail_alloc_at=2)
    with pytest.raises(Boom, match="alloc"):
        with w.scope() as s:
            for _ in range(4):
                s.alloc(8)
    assert len(w.bufs) == 2 and w.live() == 0


def test_release_hands_over_and_free_ends_early():
    w = FakeWorker()
    with w.scope() as s:
        a, b, c = s.alloc(8), s.alloc(8), s.alloc(8)
        assert s.release(b) is b
        s.free(a)
        assert a.ptr is None and w.live() == 2
        with pytest.raises(ValueError):
            s.release(b)                              # not the scope's any more
    assert c.ptr is None and b.ptr and w.live() == 1 and [x.frees for x in w.bufs] == [1, 0, 1]
    b.free()


def test_close_twice_is_fine():
    w = FakeWorker()
    s = w.scope()
    s.alloc(8), s.alloc(8)
    s.close()
    s.close()
    assert [x.frees for x in w.bufs] == [1, 1]
    s.alloc(8)                                        # a closed scope is an empty scope
    s.close()
    assert w.live() == 0


def test_a_raising_free_does_not_strand_the_others_and_its_error_surfaces():
    w = FakeWorker()
    s = w.scope()
    bufs = [s.alloc(8) for _ in range(4)]
    w.fail_free = [bufs[1], bufs[2]]
    with pytest.raises(Boom, match="free 1"):         # the first error, once the rest is freed
        s.close()
    assert [b.ptr is None for b in bufs] == [True, False, False, True]
    w.fail_free = []
    s.close()                                         # the scope forgot them all: the two that would not go are the caller's to report
    assert w.live() == 2


def test_closing_on_error_closes_only_when_the_block_raises():
    w = FakeWorker()
    s = w.scope()
    with closing_on_error(s) as same:
        assert same is s
        s.alloc(8)
    assert w.live() == 1
    with pytest.raises(Boom, match="late"):
        with closing_on_error(s):
            s.alloc(8)
            raise Boom("late")
    assert w.live() == 0
