"""What the GPU test files share: the old-style tolerances, the `dev` fixture, the measures of the bf16-faithful tier (tests/bf16_ref.py),
the child-process runner for tests whose environment switches are read once per process, the harvest of device kernel names, and
the workspace-state helpers (fills for memory of any contents, the recorder of the pool's traffic: tests/test_gpu_workspace_state.py),
and the two stream helpers of tests/test_gpu_concurrency.py (a gate that holds a stream back, and the check that two streams overlap).

A plain module, not a conftest: it defines no pytest hooks, and a test file imports what it uses by name, the fixtures included.  The
test files keep their cases, their bounds and their comparisons.  Importing this module must not initialise the GPU: the children of
run_child import it before they set anything up.
"""
import json
import math
import os
import sys
import time

import numpy as np
import pytest
import torch
from torch.autograd import DeviceType
from torch.profiler import ProfilerActivity, profile

import conftest
import recipe as R
from conftest import rel_l2

# bf16 MFMA operands against an all-fp32 / fp64 reference (test_gpu_parity.py's docstring states where each applies)
OUT_RTOL = 2e-2
GRAD_RTOL = 4e-2
RELU_GRAD_RTOL = 9e-2          # measured worst over the suite 6.5e-2 (ffn_d128 dw_1.bias), x 1.3
CCC_MIN = 1 - 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tmp_dir(request, tmp_path_factory):
    return tmp_path_factory.mktemp(request.module.__name__)


def mta():
    import multimodal_transformer_amd as m
    return m


def _report(tag, got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    r = rel_l2(got, ref)
    print("%-44s rel_l2 %.3e  max_abs %.3e  ref_rms %.3e" % (tag, r, np.abs(got - ref).max(), np.sqrt((ref ** 2).mean())))
    return r


def load_named(model, seed=R.SEED):
    """the recipe's parameters for the model's state_dict, loaded into it -> the fp32 parameters"""
    p32 = R.gen_params(R.shapes_of(model.state_dict()), seed)
    model.load_state_dict(p32)
    return p32


def seeded_encoder(d, h, n, dev, seed):
    """an n-layer Encoder with the recipe's parameters, on the device in eval mode -> (encoder, the fp32 parameters)"""
    MT = mta().multiTransformer
    enc = MT.Encoder(MT.EncoderLayer(d, MT.MultiHeadedAttention(h, d), MT.PositionwiseFeedForward(d, R.D_FF, 0.1), 0.1), n)
    p32 = load_named(enc, seed)
    return enc.to(dev).eval(), p32


# ------------------------------------------------------------------------------------------------ measures of the bf16-faithful tier
def _rows(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, 1) if a.ndim == 1 else a.reshape(-1, a.shape[-1]) if a.ndim > 2 else a


def measures(got, ref):
    """(rel-L2, per-row maximum) of got against ref."""
    g, r = _rows(got), _rows(ref)
    diff = np.linalg.norm(g - r, axis=1)
    rms = np.sqrt(np.mean(np.sum(r * r, axis=1)))
    return float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-300)), float(diff.max() / max(rms, 1e-300))


def check(tag, got, ref, rel_bound, row_bound=None, scale_ref=None, failures=None):
    """scale_ref: measure against another tensor's magnitude (for an analytically zero reference, e.g. the key bias's gradient).
    failures: a list to append a failure message to instead of raising (every tensor of a case is then reported)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rel, row = measures(got, ref)
    if scale_ref is not None:
        s = np.asarray(scale_ref, dtype=np.float64)
        rel = float(np.linalg.norm(got - ref) / np.linalg.norm(s))
        row = float(np.abs(got - ref).max() / np.sqrt(np.mean(s * s)))
    print("%-52s rel-L2 %.2e  row-max %.2e" % (tag, rel, row))
    msg = None
    if not np.isfinite(got).all():
        msg = "%s: not finite" % tag
    elif rel > rel_bound:
        msg = "%s: rel-L2 %.3e > %.1e" % (tag, rel, rel_bound)
    elif row_bound is not None and row > row_bound:
        msg = "%s: per-row maximum %.3e > %.1e" % (tag, row, row_bound)
    if msg and failures is None:
        raise AssertionError(msg)
    if msg:
        failures.append(msg)


def seq_max(got, ref):
    """max_b ||got[:, b] - ref[:, b]|| / rms_b ||ref[:, b]|| of (T, B, ...) tensors: the worst single sequence across all t."""
    g = np.asarray(got, dtype=np.float64)
    r = np.asarray(ref, dtype=np.float64)
    g, r = g.reshape(g.shape[0], g.shape[1], -1), r.reshape(r.shape[0], r.shape[1], -1)
    diff = np.sqrt(((g - r) ** 2).sum(axis=(0, 2)))
    return float(diff.max() / max(np.sqrt((r * r).sum(axis=(0, 2)).mean()), 1e-300))


def ls_scale(got, ref):
    """<got - ref, ref> / <ref, ref>: a wrongly scaled term moves it, noise hardly does."""
    r = np.asarray(ref, dtype=np.float64).ravel()
    return float(np.dot(np.asarray(got, dtype=np.float64).ravel() - r, r) / np.dot(r, r))


def check_scan(tag, got, ref, bounds, failures, seq=False, scale=None):
    """rel-L2 and per-row maximum through check(); with seq the per-sequence maximum, with scale (its bound) the least-squares scale."""
    check(tag, got, ref, bounds[0], bounds[1], failures=failures)
    if seq:
        s = seq_max(got, ref)
        print("%-52s seq-max %.2e" % (tag, s))
        if s > bounds[2]:
            failures.append("%s: per-sequence maximum %.3e > %.1e" % (tag, s, bounds[2]))
    if scale is not None:
        s = ls_scale(got, ref)
        print("%-52s scale %.2e" % (tag, s))
        if abs(s) > scale:
            failures.append("%s: least-squares scale %.3e > %.1e" % (tag, s, scale))


# the affine map's shapes (M, K, N, act, rowscale), inputs and bound: test_gpu_bf16_faithful.py and test_gpu_bf16_frontend.py run them
LIN_REL = 3e-6                       # 1.6e-7 / 7.2e-7 (fp32 accumulation only), rel-L2 and per row
_LIN = [(1, 4, 1, 0, False), (31, 5, 5, 1, False), (32, 43, 129, 0, True), (33, 301, 256, 1, True), (200, 576, 129, 1, False),
        (200, 43, 256, 0, False), (33, 576, 1, 0, True), (1, 301, 129, 1, False), (32, 4, 256, 1, True), (200, 5, 5, 0, True),
        (31, 576, 256, 0, False), (200, 301, 1, 1, True)]


def _lin_inputs(M, K, N, tag):
    x = R.gen_normal(tag + "x", (M, K), 5)
    W = R.gen_normal(tag + "w", (N, K), 5) / np.sqrt(K)
    b = 0.1 * R.gen_normal(tag + "b", (N,), 5)
    g = R.gen_normal(tag + "g", (M, N), 5)
    return x, W, b, g


# ------------------------------------------------------------------------------------------------ child processes
_RUNS = {}


def run_child(module, kind, switch, payload, tmp_dir, switches, timeout):
    """child_main(kind, out_path, json of payload) of the test module `module`, in a fresh process (conftest.run_in_fresh_process) with
    the variables of every set in `switches` removed from the environment and those of switches[switch] set -> the arrays of the .npz
    it wrote, as a dict.  One run per (module, kind, switch): later calls get the first one's arrays."""
    key = (module, kind, switch)
    if key not in _RUNS:
        env = dict(os.environ)
        for s in switches.values():
            for k in s:
                env.pop(k, None)
        env.update(switches[switch])
        env["PYTHONPATH"] = os.pathsep.join([conftest.ROOT, os.path.join(conftest.ROOT, "tests"), conftest.GOLDEN,
                                             env.get("PYTHONPATH", "")])
        out = os.path.join(str(tmp_dir), "%s_%s.npz" % (kind, switch))
        stub = "import sys, %s as m; m.child_main(*sys.argv[1:])" % module
        res = conftest.run_in_fresh_process([sys.executable, "-c", stub, kind, out, json.dumps(payload)], env, timeout=timeout)
        if res is None:
            pytest.skip("no launcher process (tests were collected with the GPU already initialised)")
        assert res["rc"] == 0, res["stderr"][-3000:]
        with np.load(out) as z:
            _RUNS[key] = {k: z[k] for k in z.files}
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ device kernel names
def device_kernel_names(fn, warm=False):
    """fn() under torch.profiler -> (its result, the names of the device kernels it launched).  The names are None where the profiler
    reports no device activity: a caller then skips only its assertion on the names.  warm: one unprofiled call of fn first."""
    if warm:
        fn()
        torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    return res, (names or None)


def library_kernels(names):
    """kernels that are not ours: ATen element-wise / reduction / copy / cat kernels, rocBLAS / hipBLASLt / MIOpen GEMMs"""
    bad = ("at::", "at_cuda", "elementwise", "Cijk_", "rocblas", "hipblas", "miopen", "MIOpen", "CatArray", "reduce_kernel", "vectorized_")
    return sorted(set(n for n in names if any(b in n for b in bad)))


# ------------------------------------------------------------------------------------------------ workspace state
# What tests/test_gpu_workspace_state.py runs every case through: a workspace's past must not show in a result.  Entries that take
# memory with any contents get it filled (FilledScratch, FilledPoolGet) and must give the same bits for every fill; entries under
# "zero once, then reuse for the same shape" get the buffer another call has just used (PoolRecorder proves that they did) and must
# give the bits of a run on a fresh pool.  tests/test_gpu_harness_cpu.py drives all of it with CPU tensors and a fake pool.
FILLS = ("zeros", "ones", "bf16_inf")      # 0x00 bytes; 0xFF bytes: a NaN in fp32 and in bf16; 16-bit words 0x7F80: +Inf in bf16 (Inf x 0 = NaN)


def fill_bytes(buf, fill):
    """Fill a contiguous uint8 tensor in place with one of FILLS -> buf.  The 16-bit pattern is little-endian from byte 0 (allocations
    are at least 2-byte aligned)."""
    assert buf.dtype == torch.uint8 and buf.dim() == 1 and fill in FILLS, (buf.dtype, buf.shape, fill)
    if fill == "zeros":
        buf.fill_(0x00)
    elif fill == "ones":
        buf.fill_(0xFF)
    else:
        buf[0::2] = 0x80
        buf[1::2] = 0x7F
    return buf


class FilledScratch:
    """Stands in for functional._scratch: the same allocation, filled with `fill`; counts its calls (a case asserts that its forward
    and its backward each made one, so that it cannot pass without the substitution having reached the entry)."""

    def __init__(self, fill):
        self.fill, self.calls = fill, 0

    def __call__(self, nbytes, device):
        self.calls += 1
        return fill_bytes(torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device), self.fill)

    def took(self):
        """the calls since the last look"""
        n, self.calls = self.calls, 0
        return n


class FilledPoolGet:
    """Stands in for a pool's get (`real`: the unwrapped one): buffers whose tag starts with `tag0` are filled with `fill` before they
    are handed out (only for an entry that documents "any contents": today mmt_local_attn_backward); counts them."""

    def __init__(self, real, fill, tag0):
        self.real, self.fill, self.tag0, self.calls = real, fill, tag0, 0

    def __call__(self, nbytes, device, tag=None):
        buf = self.real(nbytes, device, tag=tag)
        if tag is not None and tag[0] == self.tag0:
            self.calls += 1
            fill_bytes(buf, self.fill)
        return buf


class PoolRecorder:
    """Wraps get / put / clear of a WorkspacePool and keeps, per phase ("fresh", "dirtier", "probe"), which buffers were handed out and
    handed back, by data_ptr.  A buffer handed out counts as reused when it was handed back since the last clear() — it then sits alive in
    the free list, so no new allocation can have its address — and the phase that handed it back is kept with it.  The buffers a phase
    handed back stay referenced here, so their bytes can be compared later (assert_dirtied)."""

    def __init__(self, pool, monkeypatch):
        self.pool, self._get, self._put, self._clear = pool, pool.get, pool.put, pool.clear
        self.current, self.log, self._returned, self._tags = None, {}, {}, {}
        monkeypatch.setattr(pool, "get", self.get)
        monkeypatch.setattr(pool, "put", self.put)
        monkeypatch.setattr(pool, "clear", self.clear)

    def phase(self, name):
        self.current = name
        self.log[name] = {"got": [], "put": [], "bufs": {}}

    def get(self, nbytes, device, tag=None):
        buf = self._get(nbytes, device, tag=tag)
        self._tags[buf.data_ptr()] = tag
        if self.current is not None:
            self.log[self.current]["got"].append((buf.data_ptr(), tag, self._returned.pop(buf.data_ptr(), None)))
        return buf

    def put(self, buf):
        self._put(buf)
        self._returned[buf.data_ptr()] = self.current
        if self.current is not None:
            self.log[self.current]["put"].append(buf.data_ptr())
            self.log[self.current]["bufs"][buf.data_ptr()] = (self._tags.get(buf.data_ptr()), buf)

    def clear(self):
        self._clear()
        self._returned.clear()

    def _got(self, phase, tags):
        return [g for g in self.log.get(phase, {"got": []})["got"] if tags is None or (g[1] is not None and g[1][0] in tags)]

    def contents(self, phase, tags=None):
        """[(tag, buffer)] the phase handed back, each buffer once, in the order of its first return"""
        return [tb for tb in self.log[phase]["bufs"].values() if tags is None or (tb[0] is not None and tb[0][0] in tags)]

    def assert_dirtied(self, clean="fresh", dirtier="dirtier", tags=None):
        """The dirtier left other bytes than the clean run in at least one buffer of a tag both used: a dirtier that leaves a workspace
        as the probe itself leaves it shows nothing -> how many buffers differ."""
        left = {}
        for tag, buf in self.contents(clean, tags):
            left.setdefault(tag, []).append(buf)
        n = sum(1 for tag, buf in self.contents(dirtier, tags)
                if tag in left and not any(b.numel() == buf.numel() and torch.equal(b, buf) for b in left[tag]))
        assert n > 0, "the dirtier left every workspace as the clean run leaves it: the case checks nothing"
        return n

    def assert_fresh(self, phase="fresh", tags=None):
        """Every buffer the phase was handed is a new allocation or one the phase itself had handed back -> how many it was handed."""
        got = self._got(phase, tags)
        assert got, "the %s run was handed no workspace%s" % (phase, "" if tags is None else " tagged %s" % sorted(tags))
        for ptr, tag, src in got:
            assert src in (None, phase), "the %s run was handed a used workspace (%s, handed back in phase %r)" % (phase, tag, src)
        return len(got)

    def assert_reused(self, dirtier="dirtier", probe="probe", tags=None):
        """The probe was handed at least one buffer (with a tag in `tags`, if given), and every one of them is a buffer the dirtier had
        handed back -> how many distinct buffers that were."""
        got = self._got(probe, tags)
        assert got, "the dirty probe was handed no workspace%s" % ("" if tags is None else " tagged %s" % sorted(tags))
        dirty = set(self.log.get(dirtier, {"put": []})["put"])
        for ptr, tag, src in got:
            assert src is not None, "the dirty probe was handed a new workspace for %s: nothing was reused" % (tag,)
            assert ptr in dirty, "the dirty probe was handed a workspace for %s that the dirtier had not used" % (tag,)
        return len({g[0] for g in got})


def same_bits(tag, a, b, failures):
    """a, b: {name: tensor or None} of two runs of one call: the same names, every tensor finite and torch.equal to its twin."""
    assert list(a) == list(b), (tag, list(a), list(b))
    for n in a:
        if a[n] is None or b[n] is None:
            if a[n] is not b[n]:
                failures.append("%s %s: one run returned None" % (tag, n))
            continue
        if not (bool(torch.isfinite(a[n]).all()) and bool(torch.isfinite(b[n]).all())):
            failures.append("%s %s: not finite" % (tag, n))
        elif not torch.equal(a[n], b[n]):
            d = (a[n].double() - b[n].double()).abs()
            failures.append("%s %s: %d of %d entries differ (max %.3e)" % (tag, n, int((d > 0).sum()), d.numel(), float(d.max())))


# ------------------------------------------------------------------------------------------------ streams
# What tests/test_gpu_concurrency.py makes ordering edges visible with.  A kernel that races with its producer usually loses the race
# and reads the right data; behind a gate the producer is late for certain, so a missing edge shows as wrong bits every time.
GATE_MS = 40.0
_GATE = {}           # str(device) -> (a, b, milliseconds of one a @ b): calibrated once per process and device


def _gate_operands(device):
    key = str(device)
    if key not in _GATE:
        a = torch.full((4096, 4096), 1.0 / 4096, dtype=torch.float32, device=device)
        b = torch.ones(4096, 4096, dtype=torch.float32, device=device)
        out = torch.empty_like(a)
        torch.mm(a, b, out=out)                                # warm-up: the library picks and loads its kernel
        torch.cuda.synchronize(device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.mm(a, b, out=out)
        e1.record()
        e1.synchronize()
        _GATE[key] = (a, b, max(float(e0.elapsed_time(e1)), 1e-3))
    return _GATE[key]


def gate(stream, ms=GATE_MS):
    """Enqueue ordinary torch work (4096 x 4096 fp32 matmuls) that lasts at least `ms` on `stream` -> an event recorded behind it.
    While `not ev.query()` nothing enqueued on `stream` after the gate has started.  A test asserts that once everything under test is
    enqueued (assert_closed): a gate that has opened by then has shown nothing, and the test fails instead of passing."""
    a, b, t = _gate_operands(stream.device)
    with torch.cuda.stream(stream):
        out = torch.empty_like(a)
        for _ in range(int(math.ceil(ms / t))):
            torch.mm(a, b, out=out)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def assert_closed(*events):
    for ev in events:
        assert not ev.query(), "gate too short: it opened before everything under test was enqueued, so the run shows nothing"


def runs_beside(a, b, ms=GATE_MS):
    """True if work on stream `b` completes while stream `a` is still behind a gate: the two overlap.  Two streams that the runtime
    maps onto one hardware queue serialise, and a race test on them would pass for the wrong reason: a test whose meaning depends on
    the overlap asserts this premise first.  Polls for at most 1 s; drains the gate before it returns."""
    ev_a = gate(a, ms)
    with torch.cuda.stream(b):
        torch.empty(64, dtype=torch.float32, device=b.device).fill_(1.0)
        ev_b = torch.cuda.Event()
        ev_b.record(b)
    end = time.monotonic() + 1.0
    beside = False
    while time.monotonic() < end:
        if ev_b.query():
            beside = not ev_a.query()
            break
        if ev_a.query():
            break
    ev_a.synchronize()
    ev_b.synchronize()
    return beside
