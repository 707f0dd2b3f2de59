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
