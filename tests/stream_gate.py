"""The instrument of test_stream_order.py: a gated sandwich around library calls on a caller's stream.

include/matgcn.h promises that every entry point, however many library streams it forks onto, leaves the caller with one
in-order stream.  A test that uploads its inputs from the host and launches tiny kernels never sees a missing edge: the
host is slower than the device, so the device runs the launches one after another anyway.  ``sandwich`` removes that
excuse.  On the caller's stream it

1. fills every float input, every output and every scratch buffer with NaN and waits for that,
2. queues a delay kernel (the gate) and records the event ``opened`` behind it,
3. copies the true inputs from staging tensors into place - ON the stream, behind the gate,
4. queues the library call(s),
5. clones the outputs and fills inputs and reusable buffers with NaN again - still on the stream,
6. asserts ``not opened.query()``: everything above was enqueued while the stream was shut, so the device gets the whole
   DAG at once and runs it as wide as its edges allow,
7. synchronises and hands the clones back for a comparison with a synchronised run.

A library stream that is not ordered behind the caller's fork reads the NaN of step 1; a launch on the wrong stream does
too; a missing join leaves the NaN prefill in the clone or lets a straggler read the NaN of step 5.

Only float DATA is poisoned.  Index data (label starts, CSR maps, pointer tables) is written and synchronised before
the gate: a mis-ordered read gives a wrong number, never an address.
"""
import contextlib
import time
from unittest import mock

import torch

NAN = float("nan")
START_MS = 20.0     # the first gate length tried
CAP_MS = 1000.0     # a condition on test time, not a measurement: a sandwich that needs more fails

# entry points that wait for the device by design (include/matgcn.h says so at each): never inside a sandwich
KNOWN_HOST_SYNCS = {
    "matgcn_series_violations": "hipDeviceSynchronize before the counter is read back (a diagnostic, not a hot path)",
    "matgcn_profile_collect": "hipEventSynchronize on every recorded launch (profiling only)",
}


class Gate:
    """The delay in front of a sandwich.  Its length is measured: ``calibrate`` times torch.cuda._sleep with events,
    ``cover`` doubles the length from START_MS until it exceeds the host time a sandwich took to enqueue, and step 6 of
    every sandwich checks that it did.  The length only grows.  GATE serves the short sandwiches of a module; a case
    that queues many calls behind one gate brings a Gate of its own, so that its length is not paid by every case after it."""
    cycles_per_ms = None      # one calibration per process
    made = []

    def __init__(self, what="the module's sandwiches"):
        self.what = what
        self.ms = START_MS
        self.sandwiches = 0
        self.longest_host_ms = 0.0
        self.last_host_ms = 0.0
        Gate.made.append(self)

    def calibrate(self):
        if Gate.cycles_per_ms is not None:
            return
        k = 2_000_000
        for _ in range(3):      # the last of three: the first pays for loading the kernel
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            torch.cuda._sleep(k)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        assert ms > 0.0, "torch.cuda._sleep(%d) took no measurable time" % k
        Gate.cycles_per_ms = k / ms
        print("[gate] torch.cuda._sleep: %.0f cycles per ms" % Gate.cycles_per_ms)

    def cover(self, host_ms):
        """grow until the gate is twice as long as a sandwich took the host to enqueue (or fail at the cap)"""
        self.longest_host_ms = max(self.longest_host_ms, host_ms)
        while self.ms < 2.0 * host_ms:
            self.grow("a sandwich took the host %.1f ms to enqueue" % host_ms)

    def grow(self, why):
        assert self.ms < CAP_MS, "a gate of %.0f ms is still too short (%s): some call waits for the device" % (self.ms, why)
        self.ms = min(2.0 * self.ms, CAP_MS)
        print("[gate] %s: length -> %.0f ms (%s)" % (self.what, self.ms, why))

    def shut(self, stream):
        """queue the delay on ``stream`` (the current one) and return the event recorded behind it"""
        self.calibrate()
        torch.cuda._sleep(int(self.ms * self.cycles_per_ms))
        opened = torch.cuda.Event()
        opened.record(stream)
        return opened

    @staticmethod
    def report():
        for g in Gate.made:
            if g.sandwiches:
                print("[gate] %s: chosen length %.0f ms over %d sandwiches; the slowest took the host %.1f ms to enqueue"
                      % (g.what, g.ms, g.sandwiches, g.longest_host_ms))


GATE = Gate()

# The HIP runtime keeps a bounded number of commands behind a stream that does not advance: measured on an MI355X at 6814
# torch fills, or 26-30 inference forwards of a two- or three-layer binding (about 235 launches each), on the null stream
# and on a side stream alike.  The call that enqueues the next command waits for the device, whoever it is (a plain
# ``fill_`` too) - a limit of the instrument, not a wait of the library.  A sequence longer than that queues its gate
# itself (Regate) and takes step 6 where the bound is reached: what lies behind that point follows at the host's pace.
# Shutting the stream a second time further on does not help: the call that exceeds the bound then waits until that
# second gate has opened as well.
COMMANDS_BEHIND_A_SHUT_STREAM = 6814


class Regate:
    """further gates inside one ``call``: ``regate()`` checks that everything since the last gate was enqueued while it
    was still shut and queues the next one; ``close()`` checks the last.  ``in_time`` holds one flag per gate."""

    def __init__(self, gate, stream):
        self.gate, self.stream = gate, torch.cuda.default_stream() if stream is None else stream
        self.opened, self.in_time = None, []

    def __call__(self):
        self.close()
        self.opened = self.gate.shut(self.stream)

    def close(self):
        if self.opened is not None:
            self.in_time.append(not self.opened.query())
            self.opened = None


def caller_streams():
    """the null stream (None) and four side streams created one after the other: the runtime hands hardware queues to
    streams round robin in creation order (include/matgcn.h, "Hardware queues"), so with four queues every library stream
    sits on a queue other than the caller's - not behind the delay kernel by accident - for at least three of the four"""
    return [None] + [torch.cuda.Stream() for _ in range(4)]


def caller_name(i):
    return "null stream" if i == 0 else "side stream %d" % i


@contextlib.contextmanager
def nan_outputs():
    """every float tensor the binding allocates for a call (outputs, partials, scratch) is filled with NaN on the
    current stream, in front of the call that writes it"""
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poisoned(t):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.is_floating_point() and t.numel():
            t.fill_(NAN)
        return t

    with mock.patch.object(torch, "empty", lambda *a, **k: poisoned(real_empty(*a, **k))), \
            mock.patch.object(torch, "empty_like", lambda *a, **k: poisoned(real_empty_like(*a, **k))):
        yield


def _tensors(x, *args):
    x = x(*args) if callable(x) else x
    return [t for t in x if t is not None]


def sandwich(stream, write_inputs, call, outputs, poison_after, *, poison_before=(), synchronous=False, gated=True,
             retry=True, gate=GATE):
    """One gated sandwich on ``stream`` (None: the null stream); returns {name: clone} of ``outputs(result)``.

    write_inputs: (destination, staging) pairs of device float tensors - or a callable returning them;
    call: () -> result, the library call(s); it may copy further staged inputs itself (d_out between forward_train and
        backward) - those go into poison_before / poison_after;
    outputs: result -> {name: tensor}, what to clone behind the call;
    poison_after: tensors (or result -> tensors) filled with NaN behind the clones, next to every destination;
    poison_before: further tensors that hold NaN before the gate (workspace, train buffer, `prepared` of a prepare);
    synchronous: no gate, a device synchronisation between all steps - the reference and the warm-up;
    gated=False: no gate and no synchronisation either - a rehearsal that measures the host's enqueue time
        (gate.last_host_ms) for Gate.cover, for a sandwich too long to find its gate by doubling;
    retry: a gate that proves too short (step 6) is doubled and the sandwich repeated - for calls that can be repeated."""
    s = torch.cuda.default_stream() if stream is None else stream
    sync = torch.cuda.synchronize if synchronous else (lambda: None)
    while True:
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            pairs = [(d, v) for d, v in _tensors(write_inputs)]
            for d, _ in pairs:
                d.fill_(NAN)
            for t in _tensors(poison_before):
                t.fill_(NAN)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opened = gate.shut(s) if gated and not synchronous else None
            for d, v in pairs:
                d.copy_(v)
            sync()
            with nan_outputs():
                result = call()
            sync()
            clones = {k: v.clone() for k, v in outputs(result).items()}
            sync()
            for d, _ in pairs:
                d.fill_(NAN)
            for t in _tensors(poison_after, result):
                t.fill_(NAN)
            host_ms = (time.perf_counter() - t0) * 1e3
            shut = opened is None or not opened.query()
        torch.cuda.synchronize()
        del result
        gate.last_host_ms = host_ms
        if opened is None:
            return clones
        gate.sandwiches += 1
        gate.longest_host_ms = max(gate.longest_host_ms, host_ms)
        if shut:
            return clones
        if not retry:
            raise AssertionError("the gate (%.0f ms) opened before the sandwich was enqueued (%.1f ms on the host): "
                                 "the case proves nothing" % (gate.ms, host_ms))
        gate.grow("the gate opened before a sandwich of %.1f ms host time was enqueued" % host_ms)


def bits_equal(a, b):
    """bit for bit, NaN payloads included"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_floating_point():
        it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))
    return bool(torch.equal(a, b))
