"""The checks of tests/gpu_harness.py still bite: each measure on inputs built to exceed exactly that measure's bound.  No GPU needed."""
import numpy as np
import pytest
import torch

import gpu_harness as H


def _ref(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape)


def test_check_raises_on_a_scaled_tensor():
    ref, bound = _ref((50, 8)), 1e-3
    H.check("scaled", ref * (1 + 0.5 * bound), ref, bound, bound)
    with pytest.raises(AssertionError, match="rel-L2"):
        H.check("scaled", ref * (1 + 2 * bound), ref, bound)


def test_check_raises_on_one_row_past_the_row_bound():
    ref = _ref((1000, 8))
    rms = np.sqrt(np.mean(np.sum(ref * ref, axis=1)))
    got = ref.copy()
    got[417, 3] += 2e-3 * rms                      # rel-L2 2e-3 / sqrt(1000) = 6.3e-5, per row 2e-3
    H.check("one row", got, ref, 1e-4)
    with pytest.raises(AssertionError, match="per-row maximum"):
        H.check("one row", got, ref, 1e-4, 1e-3)


def test_check_raises_on_a_nan():
    ref = _ref((50, 8))
    got = ref.copy()
    got[7, 2] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        H.check("nan", got, ref, 1.0, 1.0)


def test_check_appends_to_failures_instead_of_raising():
    ref, failures = _ref((50, 8)), []
    H.check("good", ref, ref, 1e-6, 1e-6, failures=failures)
    assert failures == []
    H.check("bad", 1.01 * ref, ref, 1e-3, failures=failures)
    H.check("worse", 1.02 * ref, ref, 1e-3, failures=failures)
    assert len(failures) == 2 and failures[0].startswith("bad: rel-L2") and failures[1].startswith("worse: rel-L2")


def test_check_scan_reports_one_wrong_sequence_that_rel_l2_passes():
    T, B, H_ = 100, 20, 8
    ref = _ref((T, B, H_))
    rms = np.sqrt(np.mean(np.sum(ref * ref, axis=2)))
    got = ref.copy()
    got[:, 5, 0] += 1.5e-3 * rms                   # sequence 5 at every t: rel-L2 1.5e-3 / sqrt(20) = 3.4e-4, per row and per sequence 1.5e-3
    bounds = (7e-4, 2e-3, 1e-3)
    failures = []
    H.check_scan("seq", got, ref, bounds, failures)
    assert failures == []
    H.check_scan("seq", got, ref, bounds, failures, seq=True)
    assert len(failures) == 1 and "per-sequence maximum" in failures[0]


def test_check_scan_reports_a_wrong_scale():
    ref = _ref((64, 32))
    failures = []
    H.check_scan("dW", ref * (1 + 1e-4), ref, (4e-3, 2.5e-2), failures)
    assert failures == []
    H.check_scan("dW", ref * (1 + 1e-4), ref, (4e-3, 2.5e-2), failures, scale=3e-5)
    assert len(failures) == 1 and "least-squares scale" in failures[0]


class _Event:
    def __init__(self, name, device_type):
        self.name, self.device_type = name, device_type


def _fake_profiler(monkeypatch, events):
    class Profile:
        def __init__(self, activities):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def events(self):
            return events
    monkeypatch.setattr(H, "profile", Profile)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)


def test_device_kernel_names_maps_an_empty_harvest_to_none(monkeypatch):
    calls = []
    fn = lambda: calls.append(1) or "result"  # noqa: E731
    _fake_profiler(monkeypatch, [])
    assert H.device_kernel_names(fn) == ("result", None)
    _fake_profiler(monkeypatch, [_Event("aten::add", H.DeviceType.CPU)])
    assert H.device_kernel_names(fn) == ("result", None)
    assert len(calls) == 2
    _fake_profiler(monkeypatch, [_Event("aten::add", H.DeviceType.CPU), _Event("lstm_scan_fwd_kernel", H.DeviceType.CUDA)])
    assert H.device_kernel_names(fn, warm=True) == ("result", ["lstm_scan_fwd_kernel"])
    assert len(calls) == 4                         # warm: one unprofiled call first


# ------------------------------------------------------------------------------------------------ workspace state
class _FakePool:
    """WorkspacePool's surface on CPU tensors; reuse=False: put() forgets the buffer, so nothing is ever handed out twice."""

    def __init__(self, reuse=True):
        self.free, self.reuse, self.keep = {}, reuse, []

    def get(self, nbytes, device, tag=None):
        lst = self.free.get((nbytes, tag))
        buf = lst.pop() if lst else torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.keep.append(buf)                       # alive to the end of the test: no address comes twice
        return buf

    def put(self, buf):
        if self.reuse:
            self.free.setdefault((buf.numel(), None if not hasattr(buf, "tag") else buf.tag), []).append(buf)

    def clear(self):
        self.free.clear()


def _call(pool, tag, nbytes=64, value=1):
    """what a pooled entry does: take a workspace, write it (every byte: `value`), hand it back"""
    buf = pool.get(nbytes, "cpu", tag=tag)
    buf.tag = tag
    buf.fill_(value)
    pool.put(buf)


def test_fill_bytes_patterns():
    buf = torch.empty(8, dtype=torch.uint8)
    assert H.fill_bytes(buf, "zeros").tolist() == [0] * 8
    assert H.fill_bytes(buf, "ones").tolist() == [255] * 8
    words = H.fill_bytes(buf, "bf16_inf").view(torch.int16)
    assert words.tolist() == [0x7F80] * 4
    assert torch.isinf(words.view(torch.bfloat16)).all() and (words.view(torch.bfloat16) > 0).all()
    assert torch.isnan(H.fill_bytes(buf, "ones").view(torch.float32)).all() and torch.isnan(buf.view(torch.bfloat16)).all()
    with pytest.raises(AssertionError):
        H.fill_bytes(buf, "garbage")


def test_filled_scratch_counts_and_fills():
    s = H.FilledScratch("ones")
    assert s.took() == 0                            # a case that asserts took() > 0 fails when the entry never asked
    a, b = s(6, "cpu"), s(0, "cpu")
    assert a.tolist() == [255] * 6 and b.numel() == 1
    assert s.took() == 2 and s.took() == 0


def test_filled_pool_get_fills_only_its_tag(monkeypatch):
    pool = _FakePool()
    f = H.FilledPoolGet(pool.get, "ones", "local_attn")
    monkeypatch.setattr(pool, "get", f)
    assert pool.get(4, "cpu", tag=("linear", 1, 2, 3)).tolist() == [0] * 4 and f.calls == 0
    assert pool.get(4, "cpu", tag=("local_attn", 1, 2, 3, 4)).tolist() == [255] * 4 and f.calls == 1


def test_pool_recorder_sees_reuse(monkeypatch):
    pool = _FakePool()
    rec = H.PoolRecorder(pool, monkeypatch)
    pool.clear()
    rec.phase("fresh")
    _call(pool, ("op", 1))
    _call(pool, ("op", 1))                          # its own buffer back from the free list: still a fresh run
    assert rec.assert_fresh() == 2
    pool.clear()
    rec.phase("dirtier")
    _call(pool, ("op", 1))
    rec.phase("probe")
    _call(pool, ("op", 1))
    assert rec.assert_reused() == 1 and rec.assert_reused(tags={"op"}) == 1


def test_pool_recorder_fails_without_reuse(monkeypatch):
    pool = _FakePool(reuse=False)
    rec = H.PoolRecorder(pool, monkeypatch)
    rec.phase("dirtier")
    _call(pool, ("op", 1))
    rec.phase("probe")
    _call(pool, ("op", 1))
    with pytest.raises(AssertionError, match="nothing was reused"):
        rec.assert_reused()


def test_pool_recorder_fails_on_another_tag_and_on_no_buffer(monkeypatch):
    pool = _FakePool()
    rec = H.PoolRecorder(pool, monkeypatch)
    rec.phase("dirtier")
    _call(pool, ("op", 2))                          # another shape: another buffer
    rec.phase("probe")
    with pytest.raises(AssertionError, match="handed no workspace"):
        rec.assert_reused()
    _call(pool, ("op", 1))
    with pytest.raises(AssertionError, match="nothing was reused"):
        rec.assert_reused()
    with pytest.raises(AssertionError, match="handed no workspace"):
        rec.assert_reused(tags={"other"})


def test_pool_recorder_fails_on_a_buffer_the_dirtier_did_not_use(monkeypatch):
    pool = _FakePool()
    rec = H.PoolRecorder(pool, monkeypatch)
    rec.phase("earlier")
    _call(pool, ("op", 1))
    rec.phase("dirtier")
    _call(pool, ("op", 2))
    rec.phase("probe")
    _call(pool, ("op", 1))                          # reused, but from a phase before the dirtier
    with pytest.raises(AssertionError, match="the dirtier had not used"):
        rec.assert_reused()


def test_pool_recorder_fails_on_a_fresh_run_without_clear(monkeypatch):
    pool = _FakePool()
    rec = H.PoolRecorder(pool, monkeypatch)
    rec.phase("dirtier")
    _call(pool, ("op", 1))
    rec.phase("fresh")                              # no pool.clear() in between
    _call(pool, ("op", 1))
    with pytest.raises(AssertionError, match="used workspace"):
        rec.assert_fresh()
    pool.clear()
    rec.phase("fresh")
    with pytest.raises(AssertionError, match="handed no workspace"):
        rec.assert_fresh()
    _call(pool, ("op", 1))
    assert rec.assert_fresh() == 1


def test_pool_recorder_fails_on_a_dirtier_that_leaves_the_clean_bytes(monkeypatch):
    pool = _FakePool()
    rec = H.PoolRecorder(pool, monkeypatch)
    pool.clear()
    rec.phase("fresh")
    _call(pool, ("op", 1))
    pool.clear()
    rec.phase("dirtier")
    _call(pool, ("op", 1))                          # the same call: the same bytes
    _call(pool, ("op", 2), value=9)                 # other bytes, but under a tag the clean run never used
    with pytest.raises(AssertionError, match="checks nothing"):
        rec.assert_dirtied()
    pool.clear()
    rec.phase("dirtier")
    _call(pool, ("op", 1), value=9)
    assert rec.assert_dirtied() == 1 and rec.assert_dirtied(tags={"op"}) == 1
    with pytest.raises(AssertionError, match="checks nothing"):
        rec.assert_dirtied(tags={"other"})


def test_same_bits_reports_a_changed_entry_and_a_nan():
    a = {"y": torch.arange(6.0), "dx": None}
    failures = []
    H.same_bits("t", a, {"y": torch.arange(6.0), "dx": None}, failures)
    assert failures == []
    b = {"y": torch.arange(6.0), "dx": None}
    b["y"][4] += 1e-6
    H.same_bits("t", a, b, failures)
    assert len(failures) == 1 and "1 of 6 entries differ" in failures[0]
    n = {"y": torch.arange(6.0), "dx": None}
    n["y"][2] = float("nan")
    H.same_bits("t", n, n, failures)                # identical bits, but not a result
    assert len(failures) == 2 and "not finite" in failures[1]
    H.same_bits("t", a, {"y": torch.arange(6.0), "dx": torch.zeros(1)}, failures)
    assert len(failures) == 3 and "None" in failures[2]
