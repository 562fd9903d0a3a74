"""One memo for the small results that the Python layer derives from a caller's tensors (degrees as ints, an int32 copy of
the indices, a checked range, ...), so that an epoch pays no host read or conversion launch for them twice.

1. An entry is valid while every source is the same tensor OBJECT (weak reference, keyed by ``id`` and checked with ``is``:
   a recycled id never hits) at the same ``_version``.  ``pin=True``, for callers that pass a fresh view each epoch: the
   source is its address, shape, strides, dtype and device at the same version, and the entry holds it, so that the address
   cannot be recycled.  A write that bypasses the version counter - ``.data``, a raw kernel, ``torch.distributed`` - is
   invisible: whoever writes like that calls :meth:`Memo.forget`.
2. A source without a version counter (inference mode) is never stored: ``make()`` runs every time.
3. A miss while the stream is being captured either raises ``_lib.first_use_under_capture(what)`` before ``make`` runs
   (``"refuse"``: the value needs a host read, or must hold something before the first replay) or runs ``make`` and stores
   nothing (``"serve"``: a tensor made by a captured op holds nothing for an eager call to find).  A hit is always served.
4. Every hit hands the value's tensors to ``_lib.keep_alive``: a captured graph outlives a bounded table.
5. At most ``capacity`` entries, the least recently used goes first; entries whose source has died go when met and on insert.
6. The memo never touches the device: no read, no allocation, no synchronisation.
"""
from __future__ import annotations

import collections
import weakref

import torch

from . import _lib

_MISS = object()


class Memo:
    """``sources`` is a tensor or a tuple of tensors (None allowed), ``key`` any hashable host value; a memo keyed on shapes
    alone passes ``()`` for the sources.  A value is anything; a tensor, or those in a tuple, are kept alive on a hit."""

    def __init__(self, what: str, capacity: int = 1, under_capture: str = "refuse", pin: bool = False) -> None:
        if under_capture not in ("refuse", "serve"):
            raise ValueError(f"under_capture must be 'refuse' or 'serve', got {under_capture!r}")
        self.what, self.capacity, self.serve, self.pin = what, int(capacity), under_capture == "serve", bool(pin)
        self._entries: collections.OrderedDict = collections.OrderedDict()     # ident -> (held sources, versions, value)

    def _identify(self, sources, key):
        """``(ident, versions, the sources that are tensors)``; ident None: a source has no version counter."""
        sources = sources if isinstance(sources, tuple) else (sources,)
        live = [s for s in sources if s is not None]
        try:
            versions = [s._version for s in live]
        except (RuntimeError, AttributeError):
            return None, None, live
        if self.pin:
            return (key, *(s if s is None else (s.data_ptr(), s.shape, s.stride(), s.dtype, s.device) for s in sources)), versions, live
        return (key, *map(id, sources)), versions, live

    def get(self, sources, key=(), default=None):
        """The value stored for ``sources`` and ``key``, or ``default``."""
        ident, versions, live = self._identify(sources, key)
        entry = self._entries.get(ident)
        if entry is None:
            return default
        if entry[1] != versions or not (self.pin or all([held() is s for held, s in zip(entry[0], live)])):
            del self._entries[ident]                # written since, or another tensor on a dead one's id
            return default
        self._entries.move_to_end(ident)
        value = entry[2]
        if _lib._KEPT_BY_CAPTURE is not None:       # (asked here: an epoch's hits pay one comparison, not a walk of the value)
            _lib.keep_alive(*(v for v in (value if isinstance(value, tuple) else (value,)) if isinstance(v, torch.Tensor)))
        return value

    def put(self, sources, value, key=()) -> None:
        """Store ``value`` - under capture too: for a value that the caller knows to be valid whenever its source is."""
        ident, versions, live = self._identify(sources, key)
        if ident is None:
            return
        entries = self._entries
        for dead in [k for k, entry in entries.items() if not self.pin and any(held() is None for held in entry[0])]:
            del entries[dead]
        entries[ident] = (live if self.pin else tuple(map(weakref.ref, live)), versions, value)
        entries.move_to_end(ident)
        while len(entries) > self.capacity:
            entries.popitem(last=False)

    def lookup(self, sources, make, key=()):
        """The stored value, or ``make()`` - stored unless rule 2 or rule 3 says otherwise."""
        value = self.get(sources, key, _MISS)
        if value is not _MISS:
            return value
        if _lib.capturing():
            if not self.serve:
                raise _lib.first_use_under_capture(self.what)
            return make()
        value = make()
        self.put(sources, value, key)
        return value

    def forget(self, tensor: torch.Tensor) -> None:
        """Drop every entry that has ``tensor`` among its sources: for a writer that the version counter does not see."""
        for ident in [k for k, entry in self._entries.items() if any((held if self.pin else held()) is tensor for held in entry[0])]:
            del self._entries[ident]

    def clear(self) -> None:
        self._entries.clear()
