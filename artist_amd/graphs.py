"""Capture an epoch once, replay it every epoch: ``EpochGraph``.

A reconstruction epoch of the scenarios ARTIST ships - a handful of heliostats, 10-100 rays, 10^4 points - is a few dozen
``autograd.Function``s and ctypes calls around kernels that together run for tens to a few hundred microseconds: the host
needs longer to enqueue the epoch than the GPU needs to run it.  ``torch.cuda.graph`` records the launches once and hands
them to the GPU in one call; this module wraps it with what the library's per-stream state asks for.

    g = artist_amd.EpochGraph(step_fn, warmup=2)      # step_fn(): forward + loss + backward(); returns tensor(s)
    for epoch in range(n):
        loss = g.replay()                             # the same static tensors every time, .grad on the parameters
        optimizer.step()                              # artist_amd.optim.Adam stays OUTSIDE the graph
"""
from __future__ import annotations

import warnings

import torch

from . import _lib, ops

__all__ = ["EpochGraph"]


def _leaves_behind(outputs) -> list:
    """The leaf tensors that ``backward()`` from ``outputs`` reaches: the ``AccumulateGrad`` nodes of their autograd graphs
    (the nodes outlive ``backward()``; only what they saved is freed)."""
    leaves, seen, todo = [], set(), [t.grad_fn for t in outputs if t.grad_fn is not None]
    while todo:
        node = todo.pop()
        if node in seen:
            continue
        seen.add(node)
        variable = getattr(node, "variable", None)
        if variable is not None:
            leaves.append(variable)
        todo.extend(fn for fn, _ in node.next_functions if fn is not None)
    return leaves


class EpochGraph:
    """``step_fn`` captured into a HIP graph on a stream of its own, after ``warmup`` (>= 1) eager runs on that stream.

    ``step_fn()`` is the caller's forward + loss + ``backward()``.  It reads parameters and inputs that live at fixed addresses
    (change them in place: ``optimizer.step()``, ``copy_``), leaves ``.grad`` on the parameters and returns a tensor or a tuple
    of tensors - loss, flux, factors, whatever the caller wants to read.  :meth:`replay` runs the captured launches on the
    caller's current stream, ordered like any other work on it, and returns the same static tensors every time; their values,
    and the parameters' ``.grad``, are those of an eager ``step_fn()`` bit for bit.  ``ops.check_async_errors`` stays the way
    to learn what only the device found out.

    ``parameters``: the tensors whose ``.grad`` the step produces.  Each warm-up run drops the gradients it produced
    (``set_to_none``), so that the captured step WRITES them; a replay overwrites, it never accumulates, and it re-attaches a
    ``.grad`` that ``zero_grad(set_to_none=True)`` took away.  Default: the leaves found behind the tensors ``step_fn``
    returns (pass them when it returns detached values only).

    The stream is private - created here, kept for the lifetime of the object, never handed out - because the library's
    persistent kernels take their work counters, window tables, part scratch and pixel accumulators per (device, stream),
    those addresses are baked into the captured launches, and "launches that share a counter are ordered by their stream"
    holds for a replayed graph only if nothing else is ever launched on the stream it was captured on.  Two ``EpochGraph``s
    have two streams and share nothing.  (torch hands its streams out of a pool of 32 per device and priority: a process
    that creates more stream objects than that is handed one of them again.)

    Fresh leaves.  A parameter's ``AccumulateGrad`` node belongs to the stream it was created on and lives as long as any
    autograd graph that reaches the parameter.  If such a graph from an earlier eager step on another stream is still alive
    (a tensor with a ``grad_fn`` kept on an object, say), the captured backward would synchronise with that stream, which
    ends the process when the capture ends.  Build the ``EpochGraph`` before the parameters' first use, or hand ``step_fn``
    fresh leaves; torch's one warning about it, when seen during the warm-up, is turned into an error.

    Refused, each with an :class:`ArtistHipError` that says what to do: a CPU device or CPU outputs (no CPU fallback),
    ``ops.record_launch_events`` switched on (its events would be recorded into the graph), a device status that is pending
    when the object is built.

    Limits.  The library keeps the stream's 32 bytes of work counters, 640 KB of window tables and 40 KB of part scratch for
    the life of the process, as it does for any stream that has traced.  ``artist_amd.optim.Adam.step()`` stays outside the
    graph: ``art_adam_step`` takes the learning rate and the step number by value and forms the bias corrections on the host,
    so a replay would repeat step 1 - it raises when the stream is capturing; the loop is ``g.replay(); optimizer.step()``.
    Constructing a tracer or drawing the sun's sample inside ``step_fn`` is not supported either: both read the device.
    After a device error that ``ops.check_async_errors`` reports, build a new graph."""

    def __init__(self, step_fn, warmup: int = 2, parameters=None, device=None) -> None:
        self._graph = self._stream = None            # (close() runs from __del__ whatever __init__ got to)
        self._kept, self._grads, self._outputs = [], [], None
        warmup = int(warmup)
        if warmup < 1:
            raise ValueError("EpochGraph needs at least one warm-up run: the first use of a stream cannot be captured")
        dev = None if device is None else torch.device(device)
        if (dev is not None and dev.type != "cuda") or not torch.cuda.is_available():
            raise _lib.ArtistHipError(f"EpochGraph captures GPU work (asked for {dev if dev is not None else 'a machine without a GPU'}); "
                                      "there is no CPU fallback")
        if dev is None or dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if ops._LAUNCH_EVENTS is not None:
            raise _lib.ArtistHipError("ops.record_launch_events is on: its events would be recorded into the graph; "
                                      "switch it off (record_launch_events(False)) before building an EpochGraph")
        self.device = dev
        with torch.cuda.device(dev):
            torch.cuda.synchronize(dev)
            code = _lib.lib().art_async_status(torch.cuda.current_stream(dev).cuda_stream, 0)
            if code != _lib.ART_OK:
                raise _lib.ArtistHipError(f"a device status is pending ({_lib.lib().art_strerror(code).decode()}): a captured trace "
                                          "call would refuse to start; look at it and clear it with ops.check_async_errors() first")
            self._stream = torch.cuda.Stream(device=dev)
            # warm-up: every piece of per-stream library state and every cache that needs a host read exists afterwards
            self._stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(self._stream), warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                for _ in range(warmup):
                    outputs = self._as_tuple(step_fn())
                    if parameters is None:
                        parameters = _leaves_behind(outputs)
                    parameters = list(parameters)
                    for p in parameters:
                        p.grad = None
                    del outputs
            if any("AccumulateGrad node's stream does not match" in str(w.message) for w in seen):
                # torch says so once per process: the documented rule (class docstring, "Fresh leaves") is the real guard
                raise _lib.ArtistHipError(
                    "a parameter of step_fn was used in an autograd graph that is still alive and was built on another stream "
                    "(its AccumulateGrad node belongs to that stream): capturing the step would pull that stream into the "
                    "capture. Build the EpochGraph before the parameter's first use, or give it a fresh leaf "
                    "(p.detach().clone().requires_grad_())")
            for w in seen:                                  # (anything else the warm-up warned about is the caller's to see)
                warnings.warn_explicit(w.message, w.category, w.filename, w.lineno)
            torch.cuda.current_stream(dev).wait_stream(self._stream)
            ops.check_async_errors(dev, clear=False)       # (what the warm-up's kernels found; synchronises)
            self._graph = torch.cuda.CUDAGraph()
            _lib._KEPT_BY_CAPTURE = self._kept
            try:
                with torch.cuda.graph(self._graph, stream=self._stream):
                    outputs = step_fn()
            finally:
                _lib._KEPT_BY_CAPTURE = None
        self._single = isinstance(outputs, torch.Tensor)
        self._outputs = self._as_tuple(outputs)
        self._grads = [(p, p.grad) for p in parameters if p.grad is not None]

    def _as_tuple(self, outputs) -> tuple:
        outputs = (outputs,) if isinstance(outputs, torch.Tensor) else tuple(outputs)
        for t in outputs:
            if not isinstance(t, torch.Tensor):
                raise TypeError("step_fn must return a tensor or a tuple of tensors")
            if t.device.type != "cuda":
                raise _lib.ArtistHipError(f"step_fn returned a tensor on {t.device}: EpochGraph captures GPU work; "
                                          "there is no CPU fallback")
        return outputs

    def replay(self):
        """Run the captured step on the current stream and return its static outputs (a tensor, or a tuple as ``step_fn``
        returned one).  Asynchronous like the eager step; the outputs are overwritten by the next replay."""
        if self._graph is None:
            raise _lib.ArtistHipError("this EpochGraph has been closed")
        for p, grad in self._grads:
            if p.grad is not grad:
                p.grad = grad
        self._graph.replay()
        return self._outputs[0] if self._single else self._outputs

    def close(self) -> None:
        """Drop the graph - with the memory of its outputs and gradients - before the stream it was captured on."""
        self._graph = None
        self._outputs = None
        self._grads = []
        self._kept = []
        self._stream = None

    def __del__(self):
        self.close()
