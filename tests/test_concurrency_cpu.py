"""The host-only parts of the multi-stream layer (tests/test_gpu_concurrency.py runs the rest on the GPU): how a batch is cut into
sub-batches, which seed a sub-batch gets, when StreamFork forks at all, and the bookkeeping of WorkspacePool on CPU tensors with
torch.cuda's streams and events replaced by fakes.  No GPU, no library.
"""
import pytest
import torch

from multimodal_transformer_amd import _lib
from multimodal_transformer_amd import functional as F


# ------------------------------------------------------------------------------------------------ sub-batches
@pytest.mark.parametrize("B", range(1, 10))
@pytest.mark.parametrize("k", range(0, 13))
def test_row_chunks_cover_the_batch_once_in_order(B, k):
    chunks = F._row_chunks(B, k)
    assert len(chunks) == max(1, min(k, B))
    assert [b for lo, hi in chunks for b in range(lo, hi)] == list(range(B))
    sizes = [hi - lo for lo, hi in chunks]
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1
    assert sizes == sorted(sizes, reverse=True)                  # the larger pieces first: (2, 2, 1) for B = 5, k = 3


def test_chunk_seed_by_value_list_and_device_seed():
    s = 123456789
    assert F._chunk_seed(s, 0, 3) == s
    assert [F._chunk_seed(s, i, 3) for i in (1, 2)] == [_lib.mix64(s, 1), _lib.mix64(s, 2)]
    assert len({s, _lib.mix64(s, 1), _lib.mix64(s, 2)}) == 3
    assert F._chunk_seed(s, 1) == _lib.mix64(s, 1)               # nsplit only matters for a DeviceSeed
    for seq in ([11, 22, 33], (11, 22, 33)):
        assert [F._chunk_seed(seq, i, 3) for i in range(3)] == [11, 22, 33]
    ds = object.__new__(_lib.DeviceSeed)                         # a stand-in: no device memory behind it
    assert F._chunk_seed(ds, 0, 1) is ds
    assert F._chunk_seed([ds, ds], 1, 2) is ds
    with pytest.raises(ValueError, match="2 sub-batch streams need a list of 2 DeviceSeeds"):
        F._chunk_seed(ds, 0, 2)
    assert F._seed_arg([ds, 7.0]) == [ds, 7] and F._seed_arg(ds) is ds


# ------------------------------------------------------------------------------------------------ fakes of torch.cuda
class _Stream:
    def __init__(self, handle, log):
        self.cuda_stream, self.log = handle, log

    def wait_event(self, ev):
        self.log.append(("wait_event", self.cuda_stream, ev))

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.cuda_stream, other.cuda_stream))


class _Cuda:
    """What _lib asks of torch.cuda: the current stream, whether it is capturing, events, new streams."""

    def __init__(self, monkeypatch):
        self.log, self.capturing, self.made = [], False, 0
        self.streams = {h: _Stream(h, self.log) for h in (0, 7, 8, 9)}
        self.current = self.streams[0]
        outer = self

        class Event:
            def __init__(self):
                self.on = []

            def record(self, stream):
                self.on.append(stream.cuda_stream)
                outer.log.append(("record", stream.cuda_stream, self))

        def new_stream(device=None):
            self.made += 1
            return self.streams.setdefault(100 + self.made, _Stream(100 + self.made, self.log))

        monkeypatch.setattr(_lib.torch.cuda, "current_stream", lambda device=None: self.current)
        monkeypatch.setattr(_lib.torch.cuda, "is_current_stream_capturing", lambda: self.capturing)
        monkeypatch.setattr(_lib.torch.cuda, "Event", Event)
        monkeypatch.setattr(_lib.torch.cuda, "Stream", new_stream)

    def on(self, handle):
        self.current = self.streams[handle]

    def took(self, kind):
        out = [e for e in self.log if e[0] == kind]
        self.log[:] = [e for e in self.log if e[0] != kind]
        return out


@pytest.fixture
def cuda(monkeypatch):
    monkeypatch.setattr(_lib, "SIDE_LANES", {})
    return _Cuda(monkeypatch)


# ------------------------------------------------------------------------------------------------ StreamFork
@pytest.mark.parametrize("n", [0, 1])
def test_fork_of_fewer_than_two_pieces_stays_on_the_callers_stream(cuda, n):
    fork = _lib.StreamFork()
    main, streams = fork.begin("cpu", n)
    assert main is cuda.current and streams == [main] * n
    assert cuda.made == 0 and fork._side == {} and _lib.SIDE_LANES == {} and cuda.log == []
    fork.end(main, streams)
    assert cuda.log == []


def test_fork_switched_off_stays_on_the_callers_stream(cuda, monkeypatch):
    fork = _lib.StreamFork("MMT_TEST_FORK")
    monkeypatch.setenv("MMT_TEST_FORK", "0")
    main, streams = fork.begin("cpu", 3)
    assert streams == [main] * 3 and cuda.made == 0 and fork._side == {} and _lib.SIDE_LANES == {} and cuda.log == []
    fork.end(main, streams)
    assert cuda.log == []                                        # nothing to join: every piece ran on the caller's stream
    monkeypatch.setenv("MMT_TEST_FORK", "1")                     # read at every call
    main, streams = fork.begin("cpu", 3)
    assert [s.cuda_stream for s in streams] == [0, 101, 102] and _lib.SIDE_LANES == {101: 1, 102: 2}
    assert cuda.took("wait_stream") == [("wait_stream", 101, 0), ("wait_stream", 102, 0)]           # fork: every side stream waits
    fork.end(main, streams)
    assert sorted(cuda.took("wait_stream")) == [("wait_stream", 0, 101), ("wait_stream", 0, 102)]   # join: the caller waits for each
    main, streams = fork.begin("cpu", 2)                         # the side streams are kept and handed out again in order
    assert [s.cuda_stream for s in streams] == [0, 101] and cuda.made == 2


def test_on_side_lane(cuda):
    fork = _lib.StreamFork()
    _, streams = fork.begin("cpu", 2)
    assert not _lib.on_side_lane("cpu")
    cuda.current = streams[1]
    assert _lib.on_side_lane("cpu")


# ------------------------------------------------------------------------------------------------ WorkspacePool
def test_pool_buffer_returns_to_its_home_key_whatever_stream_puts_it(cuda):
    pool = _lib.WorkspacePool()
    a = pool.get(64, "cpu", tag=("t", 1))
    assert a.dtype == torch.uint8 and a.numel() == 64 and not a.any()
    cuda.on(7)
    _lib.SIDE_LANES[7] = 1
    pool.put(a)                                                  # handed back under a side lane's stream
    assert pool.get(64, "cpu", tag=("t", 1)) is not a            # lane 1 has no buffer of its own yet
    cuda.on(0)
    assert pool.get(64, "cpu", tag=("t", 1)) is a                # it went home, to lane 0
    assert pool.get(64, "cpu", tag=("t", 1)) is not a            # and is handed out once
    pool.put(torch.zeros(64, dtype=torch.uint8))                 # a buffer the pool never handed out is not taken in
    assert all(not v for v in pool._free.values())


def test_pool_lanes_sizes_and_tags_never_mix(cuda):
    pool = _lib.WorkspacePool()
    _lib.SIDE_LANES.update({7: 1, 8: 2})
    held = {}
    for h in (0, 7, 8):
        cuda.on(h)
        held[h] = pool.get(32, "cpu", tag=("t",))
    for h in (8, 0, 7):
        cuda.on(h)
        pool.put(held[h])
    for h in (7, 8, 0):
        cuda.on(h)
        assert pool.get(32, "cpu", tag=("t",)) is held[h]
        pool.put(held[h])
        assert pool.get(32, "cpu", tag=("u",)) is not held[h]    # same bytes, another tag: another layout inside
        assert pool.get(33, "cpu", tag=("t",)) is not held[h]
    cuda.on(9)                                                   # a stream StreamFork does not know is lane 0
    assert pool.get(32, "cpu", tag=("t",)) is held[0]
    pool.clear()
    assert pool._free == {} and pool._home == {} and pool._last == {}


def test_pool_orders_two_streams_of_one_lane(cuda):
    pool = _lib.WorkspacePool()
    cuda.on(7)
    a = pool.get(16, "cpu", tag=("t",))
    (fill,) = cuda.took("record")                                # behind the zero fill of a new buffer
    assert fill[1] == 7 and cuda.log == []
    pool.put(a)
    (back,) = cuda.took("record")
    assert back[1] == 7 and pool._last[a.data_ptr()][0] == 7
    assert pool.get(16, "cpu", tag=("t",)) is a and cuda.log == []          # the same stream again: its own order is the order
    pool.put(a)
    ev = cuda.took("record")[0][2]
    cuda.on(9)
    assert pool.get(16, "cpu", tag=("t",)) is a
    assert cuda.took("wait_event") == [("wait_event", 9, ev)] and ev.on[-1] == 7       # stream 9 waits for what stream 7 queued
    pool.put(a)
    assert cuda.took("record")[0][1] == 9 and pool._last[a.data_ptr()][0] == 9
    cuda.on(7)
    assert pool.get(16, "cpu", tag=("t",)) is a
    assert [e[:2] for e in cuda.took("wait_event")] == [("wait_event", 7)]             # and back


def test_pool_under_capture_neither_records_nor_waits(cuda):
    pool = _lib.WorkspacePool()
    a = pool.get(16, "cpu", tag=("t",))
    pool.put(a)                                                  # the eager warm-up, on stream 0
    stamp = pool._last[a.data_ptr()]
    cuda.log.clear()
    cuda.on(8)
    cuda.capturing = True
    assert pool.get(16, "cpu", tag=("t",)) is a                  # the capture finds the warm-up's buffer: no allocation
    pool.put(a)
    b = pool.get(24, "cpu", tag=("t",))                          # and one it has to create is not stamped either
    assert cuda.log == [] and pool._last[a.data_ptr()] is stamp and b.data_ptr() not in pool._last
    cuda.capturing = False
    cuda.on(0)
    assert pool.get(16, "cpu", tag=("t",)) is a and cuda.log == []          # the stamp of its last eager use: the same stream
